// arx_kernels.hpp -- host-callable launchers for the HIP kernels (libarx.so internals).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "arx_layout.hpp"

struct arx_acoustics;  // include/arx.h

namespace arx {

// ---- the trace program (arx_trace.hip; the query's device code: arx_trace_device.hpp) ----
// Trace kernel (raygen + traversal + closest-hit + histogram, fused) over rays
// [a.ray_begin, a.ray_end); cus = compute units of the device (persistent grid size).
// Quantized nodes when a.qnodes is set, else the f32 coded nodes; the global-memory stack when
// the tree is deeper than the LDS stack or force_global_stack (a parity hook).
// fill_dirs false: a.dirs already holds this launch's directions (kept from an earlier launch of the same
// seed and ray range, in any order of the pool's slots); the pre-pass then only clears and resets
// the pool cursor.  With a.cost set, a launch that takes the pool on the 16-bit LDS-stack instance
// (trace_can_measure) runs its measuring instance; every other launch ignores it.
hipError_t launch_trace(const TraceArgs& a, int cus, hipStream_t s, bool force_global_stack = false,
                        bool fill_dirs = true);
bool trace_can_measure(const TraceArgs& a, int cus, bool force_global_stack);
// The pool's share of a launch's rays in this build, in 1/256 (pool_static_rays' dyn_share).
uint32_t trace_pool_share();
// Longest-first pool: dirs_out = dirs_in with the pool's slots [pool_static_rays(n, trace_pool_share()), n)
// permuted by descending cost (the measuring launch's a.cost) and the static slots copied; bins:
// order_bins_bytes() of device scratch.  All on s, nothing waits on the host.
hipError_t launch_order_pool(const void* dirs_in, void* dirs_out, const unsigned short* cost, uint32_t* bins, uint64_t n,
                             hipStream_t s);
size_t order_bins_bytes();
// The path cache's recording (arx_renderer::PathCache).  trace_can_cache: the launch takes a 16-bit LDS-stack
// instance, pool or small -- the ones with a recording instance.  launch_path_record: that instance's
// recording twin over the scene alone, on a.dirs as it stands (no directions are made), storing every
// query's closest hit into a.rec; a.counters (a.clear_counters of them zeroed first)
// and a.cursor must be a scratch block, a.hist is not touched.
bool trace_can_cache(const TraceArgs& a, bool force_global_stack);
hipError_t launch_path_record(const TraceArgs& a, int cus, hipStream_t s);
// Nodes below this index are answered by the trace kernels' LDS copy (0: this build has none).
int32_t trace_node_cache();
// Lanes of the largest persistent trace grid (columns of the global traversal stack).
inline uint64_t trace_max_lanes(int cus) { return (uint64_t)(cus > 0 ? cus : 256) * 2048ull; }
// i64 histogram -> f32 IR (+ mono merge); unit = e0 * 2^-frac_bits.
hipError_t launch_finalize_ir(const long long* hist, float* ir_left, float* ir_right, int32_t ir_len,
                              double unit, int32_t is_mono, hipStream_t s);
// dst[i] += src[i], i < n (int64 histogram bins).
hipError_t launch_hist_add(long long* dst, const long long* src, uint64_t n, hipStream_t s);
hipError_t launch_clear(unsigned long long* hist, uint64_t n, unsigned long long* counters, int n_counters,
                        hipStream_t s);
hipError_t launch_ray_directions(uint64_t seed, uint64_t first, uint64_t count, float* d_out, hipStream_t s);
// Register allocation of the production trace kernel instance (hipFuncGetAttributes numRegs), the
// waves per SIMD it admits, and the waves per SIMD the persistent grid is sized for.
// Register allocation of the LDS-stack trace instance of node format fmt, the large-launch (ray pool)
// or the small-launch one (small), and which of the two launch_trace takes for these arguments.
constexpr int kInstPool = 0, kInstSmall = 1, kInstMeasure = 2;  // the pool's measuring instance (16-bit nodes only)
hipError_t trace_kernel_occupancy(int fmt, int instance, int* vgprs, int* waves_admitted, int* waves_target);
bool trace_uses_small_block(const TraceArgs& a, int cus, bool force_global_stack);
// identity of the trace kernel in this build (build.py trace_source_id; arx_trace_kernel_id)
uint64_t trace_kernel_source_id();

// ---- the replay family (arx_replay.hip): frames from launch_path_record's records ----
// launch_path_replay: the frame from those records and the receiver sub-tree (replay_kernel), with the
// clear a.clear_bins / a.clear_counters ask for in front; a.dirs must be the buffer the records were made on.
hipError_t launch_path_replay(const TraceArgs& a, hipStream_t s);
// The filtered replay of a recording that stored its queries' start state (a.gstack of
// launch_path_record pointed at the filter's planes, arx_layout.hpp): the clear, filter_kernel over
// every slot, replay_cand_kernel over the candidates it listed.  max_bounces in [1, kFilterMaxBounces];
// f.list and f.heads belong to the frame set whose stream s is.  Results are launch_path_replay's.
hipError_t launch_path_replay_filtered(const TraceArgs& a, const FilterArgs& f, hipStream_t s);
// The filtered replay for a chunk of `listeners` table entries at once (filter_multi_kernel: one read of the
// segment plane serves kListenerFilterWidth listeners; replay_cand_multi_kernel: one launch for the whole
// chunk).  a is the replay's arguments (dirs and rec the cache's); its hist, counters and center and f's
// list and heads are taken from each entry instead, the box from the entry's top node in a.cnodes.  Per
// listener the results are launch_path_replay_filtered's.  No clear: the caller clears the chunk's block.
hipError_t launch_listeners_replay(const TraceArgs& a, const FilterArgs& f, const ListenerEntry* d_table,
                                   int32_t listeners, hipStream_t s);

// ---- room-acoustic parameters (arx_acoustics.hip): decay curves and ISO 3382-1 statistics ----
constexpr int kScanWorkgroup = 1, kScanTiled = 2;  // arx_debug_set_scan_shape
constexpr int kScanDefault = kScanTiled;  // 7x faster at 96 000 bins
struct AcousticsArgs {
    const long long* hist;  // 2*n: [L | R]
    int32_t n;              // ir_len
    int32_t sample_rate;
    double unit;            // e0 * 2^-frac_bits, copied into the results
    long long* edc;         // out: 3*n, channels L, R, L + R
    ::arx_acoustics* out;   // out: 3 results
    void* scratch;          // acoustics_scratch_bytes()
    int shape;              // kScanWorkgroup or kScanTiled
};
size_t acoustics_scratch_bytes();
// Scan (one or two launches), fit partials, results: all on s, nothing waits on the host.
hipError_t launch_acoustics(const AcousticsArgs& a, hipStream_t s);

// ---- moving listener (arx_receiver.hip): transform + fixed-topology refit of the receiver ----
struct RefitArgs {
    const TriRec* local_tris;   // receiver triangles in leaf order, local frame (ids, absorption set)
    int32_t n_tris;
    int32_t tri_base;           // global TriRec index of the first receiver triangle
    const BvhNode* local_nodes; // receiver sub-tree (relocated: global refs), boxes unused
    int32_t n_nodes;
    int32_t node_base;          // global node index of local node 0
    const int32_t* level_nodes; // local node indices, deepest level first
    const int32_t* level_start; // [n_levels + 1] offsets into level_nodes
    int32_t n_levels;
    int32_t root_ref, root_count;  // the receiver root as a child reference (global)
    float m[9];                 // rotation, row-major in place_vertices' order (r00 r10 r20, r01 r11 r21, r02 r12 r22)
    float t[3];                 // listener position
    float pad;                  // box padding (>= the builder's 1e-5 * max|coordinate|)
    QGrid grid;
    TriRec* tris;               // outputs
    BvhNode* cnodes;
    QNode2* qnodes;             // null: the quantized copy is not maintained (receiver off the grid)
    unsigned int* flag;         // raised to flag_value if a box fell off the grid (never, given the host's bound)
    unsigned int flag_value;    // the tree write's generation (arx_renderer::tree_gen)
    // CW4 copy (null wbuf: not maintained): the receiver's CW4 nodes (11 ints each: the BVH2
    // (ref, count) of the 4 slots, meta, base, self unit), its leaf triangles ((unit, local index)
    // pairs) and the top node (unit 0: child 0 = the scene root, unit 2; child 1 = the receiver
    // root, unit 4)
    uint4* wbuf;
    const int32_t* w4_nodes;
    int32_t n_w4;
    const int32_t* w4_tris;
    int32_t n_w4_tris;
    float scene_lo[3], scene_hi[3];
    int32_t scene_nonempty;
};
size_t receiver_refit_lds(int32_t n_tris, int32_t n_nodes, int32_t n_levels);  // bytes of LDS
hipError_t launch_receiver_refit(const RefitArgs& a, hipStream_t s);
// A chunk of listeners (arx_render_listeners): block j refits the receiver at d_table[j]'s pose into that
// entry's slot and writes its top node; a's own m / t / pad are not used, and there is no CW4 copy.
hipError_t launch_receiver_refit_multi(const RefitArgs& a, const ListenerEntry* d_table, int32_t listeners, hipStream_t s);
// The quantized copy of nodes [0, n) re-made on the device from the coded f32 nodes for grid g
// (quantize_nodes16's arithmetic, bit for bit): a new scene or a grown grid costs one launch and
// no host work or upload.  *flag is raised to flag_value (atomic max) if a box falls off the grid.
hipError_t launch_requant16(const BvhNode* coded, uint64_t n, const QGrid& g, QNode2* out, unsigned int* flag,
                            unsigned int flag_value, hipStream_t s);
// The CW4 nodes of n f32 node records (W4NodeF: top node, scene, host-built receiver) quantized for
// grid g into the CW4 buffer at their own units (quantize_w4, arx_wide.hpp).
hipError_t launch_requant_w4(const W4NodeF* nodes, uint64_t n, const QGrid& g, uint4* wbuf, unsigned int* flag,
                             unsigned int flag_value, hipStream_t s);

// ---- convolution (arx_conv.hip; its kernels: arx_conv_kernels.hpp, arx_conv_fft.hpp) ----
struct ConvPlan;  // opaque, defined in arx_conv.hip
ConvPlan* conv_plan_create(int32_t ir_len, int32_t sample_rate, int device, char* err, size_t errlen);
void conv_plan_destroy(ConvPlan* p);
// Spectra of the two IRs (device f32, ir_len each), kept for the following conv_run calls.
hipError_t conv_set_ir(ConvPlan* p, const float* d_ir_left, const float* d_ir_right, hipStream_t s);
// Device-resident file-mode convolution (kernels.cu:382-438 + AudioRenderer.cpp:706-711).  With
// d_ir_left / d_ir_right the IR spectra are recomputed from them first (on the direct path inside
// the audio's own column pass); with NULLs the spectra of the last conv_set_ir are used.
hipError_t conv_run(ConvPlan* p, const float* d_in, int64_t n_frames, float* d_out_left, float* d_out_right,
                    const float* d_ir_left, const float* d_ir_right, hipStream_t s);
// A time-block shard of conv_run: the one-second block pairs [pair_begin, pair_end) of the file
// (clamped), writing the output frames those pairs own (arx_group_conv_shard) -- bit-identical to the
// same frames of conv_run.  Plans without the chained pass C (conv_plan_shards false) convolve and
// write the whole file.
hipError_t conv_run_pairs(ConvPlan* p, const float* d_in, int64_t n_frames, float* d_out_left, float* d_out_right,
                          const float* d_ir_left, const float* d_ir_right, int64_t pair_begin, int64_t pair_end,
                          hipStream_t s);
bool conv_plan_shards(const ConvPlan* p);
const char* conv_plan_describe(const ConvPlan* p);
// Input reuse: conv_prepare_input transforms a file's blocks once (kept in the plan until the next
// conv_run or conv_prepare_input); conv_run_prepared convolves them with the current IR (new spectra
// from d_ir_left / d_ir_right when given), bit-identical to conv_run on the same input.
hipError_t conv_prepare_input(ConvPlan* p, const float* d_in, int64_t n_frames, hipStream_t s);
hipError_t conv_run_prepared(ConvPlan* p, float* d_out_left, float* d_out_right, const float* d_ir_left,
                             const float* d_ir_right, hipStream_t s);
bool conv_has_prepared(const ConvPlan* p);
int64_t conv_prepared_frames(const ConvPlan* p);
// Live (mic) block: plans created with sample_rate = block length.  One block of n_in <= block
// f64 samples, circular length-ir_len convolution with both IR spectra, / (ir_len/2), zipped
// L/R into 2*ir_len doubles (AudioRenderer.cpp:593-651, kernels.cu:345-377, 450-487).
hipError_t conv_run_live(ConvPlan* p, const double* d_in, int64_t n_in, double* d_out_interleaved, hipStream_t s);
int32_t conv_plan_block(const ConvPlan* p);
// identity of the convolution kernels in this build (arx_conv_kernel_id): build.py conv_source_id's
// hash of the kernel headers, which the stored traffic profile that bench.py reads must match --
// host-only edits of arx_conv.hip leave it, and the profile, valid
uint64_t conv_kernel_source_id();

// ---- streaming convolution (arx_conv_stream.hip): uniformly partitioned overlap-save, f64 ----
struct StreamPlan;  // opaque
// block: frames per callback (<= 4096); FFT size = the power of two >= 2*block.
StreamPlan* stream_plan_create(int32_t ir_len, int32_t block, int device, char* err, size_t errlen);
void stream_plan_destroy(StreamPlan* p);
hipError_t stream_reset(StreamPlan* p, hipStream_t s);                      // zero history + delay line
// Partition spectra of a new IR into the current set.  keep_previous (needs stream_set_fade): the
// set the last block used is kept as the previous one (a pointer swap) and the other is rebuilt.
hipError_t stream_set_ir(StreamPlan* p, const float* d_ir_left, const float* d_ir_right, bool keep_previous,
                         hipStream_t s);
// One block (n_in <= block f64 frames, zero padded) -> 2*block zipped L/R doubles.
hipError_t stream_run(StreamPlan* p, const double* d_in, int64_t n_in, double* d_out_interleaved, hipStream_t s);
// Crossfade of fade_frames in [0, block] frames with the weights h_w[0..fade_frames) of the current
// set (0: off, h_w unused).  The first fade allocates the previous set and the weight table
// (hipErrorOutOfMemory); the table is uploaded on s.
hipError_t stream_set_fade(StreamPlan* p, int32_t fade_frames, const double* h_w, hipStream_t s);
// A transition block: stream_run with both sets, frame i < fade as fma(w[i], y_cur - y_prev, y_prev).
hipError_t stream_run_xfade(StreamPlan* p, const double* d_in, int64_t n_in, double* d_out_interleaved,
                            hipStream_t s);
int32_t stream_plan_block(const StreamPlan* p);
int64_t stream_plan_blocks(const StreamPlan* p);  // processed since the last reset
int32_t stream_plan_fade(const StreamPlan* p);
int32_t stream_plan_partitions(const StreamPlan* p);
int32_t stream_plan_fft(const StreamPlan* p);

// ---- walk-through convolution (arx_conv_walk.hip): a signal against a per-block IR schedule ----
// The scratch of one call, as byte offsets (each part rounded up to 256 B; arx_debug_walk_bytes is
// `total`), with the stream plan's sizes for ir_len frames in blocks of `block`.
struct WalkLayout {
    int32_t B, N, lgN, P;
    double scale;
    uint64_t tw;      // N twiddles (16 B each)
    uint64_t w;       // fade weights (f64)
    uint64_t G;       // irs_used x P x N partition spectra
    uint64_t X;       // n_blocks x N input spectra
    uint64_t Z;       // (n_blocks + n_transitions) x N accumulated spectra, one per item
    uint64_t yprev;   // n_transitions x 2 fade: the previous IR's faded frames, zipped
    uint64_t irs;     // irs_used x ir_len f32 left, then as many right
    uint64_t in;      // n_blocks x block f64 input frames
    uint64_t out;     // n_blocks x 2 block f64 output frames, zipped
    uint64_t tables;  // per item its block, IR slot and transition (-1: none), then per transition its block (int32)
    uint64_t total;
};
WalkLayout walk_layout(int32_t ir_len, int32_t block, uint64_t irs_used, uint64_t n_blocks, uint64_t n_transitions,
                       int32_t fade);
// W_N^e as 2 N doubles: what the scratch's `tw` must hold.
void walk_twiddle_table(int32_t N, std::vector<double>& out);
// X rows the MAC's LDS ring holds for a tile of this many items (the launch's LDS: rows x 4 KiB).
int32_t walk_tile_rows(int32_t tile);
struct WalkArgs {
    void* scratch;       // laid out by `layout`; tw, w, irs, in and tables filled, out written
    WalkLayout layout;
    int32_t ir_len;
    int64_t n_frames;    // input frames in `in`, <= n_blocks * B
    int32_t n_blocks, n_transitions, n_used;
    int32_t fade;        // frames blended on a transition block (unused without one)
    int32_t tile;        // items per MAC workgroup, >= 1
};
// The five launches (IR spectra, forward, MAC, inverse, blend) on s; nothing waits on the host.
hipError_t launch_walk(const WalkArgs& a, hipStream_t s);

// ---- band synthesis (arx_band_synth.hip): one broadband IR pair from the band IRs ----
// out[n] = (float) sum_b sum_k g_b[k] * ir_b[n + c - k], c = (taps - 1) / 2, in include/arx.h's order
// (arx_combine_bands): per band one f64 accumulator, taps ascending, an explicit fma each; the bands' sums
// added in band order; one rounding to f32.  Samples outside [0, ir_len) read as zero.
struct BandSynthArgs {
    const float* ir_left;    // n_bands x ir_len
    const float* ir_right;
    const double* filters;   // n_bands x taps
    float* out_left;         // ir_len
    float* out_right;
    int64_t ir_len;          // 1 .. INT32_MAX
    int32_t n_bands;         // 1 .. kMaxBands
    int32_t taps;            // odd, 1 .. ARX_BAND_TAPS_MAX
};
hipError_t launch_band_synth(const BandSynthArgs& a, hipStream_t s);

}  // namespace arx
