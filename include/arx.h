/*
 * arx.h -- C ABI of the MI355X acoustic impulse-response engine (libarx.so).
 *
 * Drop-in boundary for the GPU path of sgrazi/AudioRenderingV2's obj_raytracer.
 * The reference exposes that path as the C++ class AudioRenderer
 * (R/prebuild/obj_raytracer/AudioRenderer.h:16-152) over free CUDA/cuFFT
 * functions (R/prebuild/obj_raytracer/kernels.cuh:17-28).  Every entry point
 * below names the reference member/function it replaces.  Plain pointers and
 * sizes only; no C++ or torch types.  Every call returns an arx_status
 * (the reference throws or exit()s: optix7.h:8-45, kernels.cu:7-68); the
 * message of the last failure on the calling thread is arx_last_error().
 *
 * Threading: one renderer is driven by one host thread at a time (the
 * reference's AudioRenderer is not thread-safe either, AudioRenderer.h; the
 * app serialises it with output_buffer_mutex, main.cpp:38-63).  All GPU work
 * is issued on the renderer's HIP stream (arx_set_stream), never the null
 * stream; calls that return host data synchronise that stream.
 */
#ifndef ARX_H
#define ARX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARX_ABI_VERSION 2

typedef enum arx_status {
    ARX_OK = 0,
    ARX_ERR_INVALID_ARGUMENT = 1,
    ARX_ERR_HIP = 2,          /* HIP runtime / kernel failure (reference: CUDA_CHECK throw) */
    ARX_ERR_OUT_OF_MEMORY = 3,
    ARX_ERR_NOT_READY = 4,    /* e.g. render before a scene was set */
    ARX_ERR_IO = 5,
    ARX_ERR_INTERNAL = 6      /* device-side invariant violated (e.g. BVH stack overflow) */
} arx_status;

typedef struct arx_renderer arx_renderer;

/* Construction parameters: Context::loadContext (R/prebuild/obj_raytracer/Context.cpp:15-236)
 * feeding AudioRenderer(model, ir_length_in_seconds, sample_rate, materials, rays)
 * (AudioRenderer.h:24) and the setters called before render (main.cpp:548-553). */
typedef struct arx_config {
    int32_t rays_x, rays_y, rays_z;     /* rays.{x,y,z}; N = x*y*z (Context.cpp:125-133) */
    uint32_t ir_length_in_seconds;      /* renderer_parameters.ir_length_in_seconds (rounded) */
    int32_t sample_rate;                /* audio file rate, 44100 in live mode (Context.cpp:197-224) */
    float base_power;                   /* pathtracer_parameters.base_power */
    float energy_thres;                 /* ray_energy_threshold */
    uint32_t max_bounces;               /* ray_max_bounces (rounded) */
    float hrtf_absorption_rate;         /* round()ed by the reference config reader (Context.cpp:145) */
    int32_t is_mono;                    /* scene_parameters.mono */
    uint64_t seed;                      /* Philox key; replaces curand_init(clock64(), tid) (devicePrograms.cu:216-217) */
    int32_t device;                     /* HIP device ordinal (reference hard-codes 0, AudioRenderer.cpp:252) */
} arx_config;

typedef struct arx_stats {
    uint64_t queries;        /* closest-hit queries issued (== optixTrace calls) */
    uint64_t receiver_hits;  /* rays terminated on a receiver half */
    uint64_t misses;         /* rays terminated by __miss__radiance */
    double trace_ms;         /* device time of the last trace kernel (HIP events) */
    double conv_ms;          /* device time of the last convolution */
    int64_t n_scene_tris, n_receiver_tris, n_nodes;
    int32_t bvh_depth;
    /* guards for stored profiles (bench.py): the scene tree's content hash (nodes + triangle
     * records of the static scene), and the production trace kernel's register allocation as the
     * runtime reports it (hipFuncGetAttributes) with the waves per SIMD it admits and the waves per
     * SIMD the persistent launch is sized for (a mismatch means the compiler changed the
     * allocation: the launch would leave SIMDs unevenly loaded) */
    uint64_t tree_hash;
    int32_t trace_vgprs;
    int32_t trace_waves_per_simd;
    int32_t trace_waves_target;
    int32_t trace_format;    /* node format of the last trace launch: 0 f32 BVH2, 1 16-bit quantized BVH2,
                              * 2 4-wide compressed (CW4) */
    int32_t trace_grid_cus;  /* CUs the last trace launch's persistent grid was sized for: the device's,
                              * or half of them for a ray-pool launch with frames in flight (its wave
                              * slots then hold two frames' launches side by side, arx_set_frames_in_flight) */
} arx_stats;

const char* arx_status_string(arx_status s);
const char* arx_last_error(void);
int arx_abi_version(void);
void arx_default_config(arx_config* cfg); /* the reference's defaults (Context.cpp:19-117) */

/* AudioRenderer::AudioRenderer (AudioRenderer.h:24; AudioRenderer.cpp:60-93):
 * allocates the IR histogram/IR buffers (ir_len = ir_length_in_seconds*sample_rate bins). */
arx_status arx_create(const arx_config* cfg, arx_renderer** out);
void arx_destroy(arx_renderer* r);
arx_status arx_get_config(const arx_renderer* r, arx_config* out);
/* Issue all work on this hipStream_t, used as given (NULL = the legacy null stream).  The
 * renderer starts on a non-blocking stream of its own; arx_get_stream returns the current one. */
arx_status arx_set_stream(arx_renderer* r, void* hip_stream);
void* arx_get_stream(const arx_renderer* r);

/* ---- Device buffers and runtime -------------------------------------------------------------
 * Small helpers so that a caller (bench.py, a C host) needs no other GPU framework for its device
 * buffers and can see which HIP / RCCL runtime libarx resolved.  No reference equivalent (its
 * CUDABuffer, CUDABuffer.h:10-68, is internal). */
int32_t arx_device_count(void); /* HIP devices visible to this process; < 0 on error */
arx_status arx_device_alloc(int32_t device, size_t bytes, void** out);
void arx_device_free(int32_t device, void* p);
/* Synchronous copy between any two of host / device memory (hipMemcpyDefault). */
arx_status arx_memcpy(int32_t device, void* dst, const void* src, size_t bytes);
/* "hip=<path of the loaded libamdhip64> (runtime version) rccl=<path of the loaded librccl>
 * (version)" into buf[len]. */
arx_status arx_runtime_info(char* buf, size_t len);
/* Scene trees built by this process so far (arx_set_scene / arx_group_set_scene): a group builds
 * its tree once and shares it between its members, and geometry identical to a scene some renderer
 * still holds reuses that build (a process-wide cache keyed by a 128-bit hash of the arrays). */
uint64_t arx_scene_build_count(void);

/* Static scene geometry: AudioRenderer::buildAccel + buildSBT (AudioRenderer.cpp:95-218, 413-464),
 * with getMaterialAbsorption (:34-56) already applied per triangle by the caller
 * (arx_material_absorption).  tri_vertices: n_tris*9 floats (P1,P2,P3 in mesh index order);
 * triangle order is the global id used to break equal-distance ties.  Builds the
 * SAH BVH on the host and uploads it (once; receivers are kept in a separate sub-tree).
 * Absorption must lie in [0, 1] (or be -1 / -2, the receiver marks): unlike the reference, which
 * takes any config value, the int64 fixed-point IR needs energies that never grow. */
arx_status arx_set_scene(arx_renderer* r, const float* tri_vertices, const float* tri_absorption,
                         int64_t n_tris);
/* The two receiver half-spheres in their local frame: HalfSphere (HalfSphere.cpp:3-31) loaded
 * from leftHalf.obj (side 0) / rightHalf.obj (side 1); n_tris*9 floats. */
arx_status arx_set_receiver_model(arx_renderer* r, int side, const float* tri_vertices_local,
                                  int64_t n_tris);
/* place_receiver_half's vertex transform alone (OptixModel.cpp:178-193): v' = (x,y,z) +
 * rotate(-radians(yaw), +Y) * v with glm's operation order; host-only, no device needed. */
arx_status arx_place_receiver_vertices(const float* local_xyz, int64_t n_vertices, float x, float y, float z,
                                       float yaw_deg, float* out_xyz);
/* getMaterialAbsorption (AudioRenderer.cpp:34-56): receiver_left -1, receiver_right -2,
 * exact name match in the config list, else 0.5. */
float arx_material_absorption(const char* name, const char* const* names, const float* absorption,
                              size_t n_materials);

/* setEmitterPosInOptix (AudioRenderer.cpp:752-756). */
arx_status arx_set_emitter(arx_renderer* r, float x, float y, float z);
/* placeReceiver + setSphereCenterInOptix (OptixModel.cpp:153-257, AudioRenderer.cpp:758-762):
 * receiver halves rotated by -yaw about +Y, translated to (x,y,z); sphere center = (x,y,z).
 * Rebuilds only the receiver sub-tree (no full rebuild, unlike reload() :466-486). */
arx_status arx_set_listener(arx_renderer* r, float x, float y, float z, float yaw_deg);
arx_status arx_set_thresholds(arx_renderer* r, float energy, uint32_t max_bounces); /* :764-768 */
arx_status arx_set_hrtf_absorption_rate(arx_renderer* r, float rate);             /* :770-773 */
arx_status arx_set_base_power(arx_renderer* r, float base_power);                 /* :775-778 */
arx_status arx_set_mono_output(arx_renderer* r, int mono);                        /* :800-803 */
arx_status arx_set_seed(arx_renderer* r, uint64_t seed);

/* AudioRenderer::render (AudioRenderer.h:27; AudioRenderer.cpp:489-523): clear, trace all
 * N rays, finalize the stereo IR (mono merge = addIRs, kernels.cu:519-527).  render_ms gets the
 * trace kernel's device time (the reference's timed window, :495-518). */
arx_status arx_render(arx_renderer* r, double* render_ms);
/* Frames in flight (n = 1 to 3; no reference equivalent -- its render() blocks, AudioRenderer.cpp:
 * 489-523).  With n > 1, consecutive render() calls rotate over n streams, histograms and IRs:
 * frame k + 1 traces while frame k's trace finishes and its IR is convolved, so a render/convolute
 * loop keeps the GPU full.  Results are those of one frame at a time, bit for bit: every getter,
 * convolution and IR copy refers to the last frame started, and the two frames meet only where they
 * share state (scene and receiver uploads wait for the other frame's trace; convolutions, IR
 * spectra and the caller's output buffers for its convolution).  A trace launch large enough for
 * the ray pool is then sized for half the CUs' wave slots (arx_stats.trace_grid_cus), so two frames'
 * launches run side by side instead of meeting only in each other's tail; a single frame
 * (arx_set_frames_in_flight(r, 1)) is therefore faster alone, a render/convolute loop faster in
 * total.  Not with arx_set_stream or arx_attach_histogram (ARX_ERR_INVALID_ARGUMENT either way
 * round). */
arx_status arx_set_frames_in_flight(arx_renderer* r, int32_t n);

/* Building blocks of render() for ray-sharded multi-GPU use (no reference equivalent; the
 * reference is single-GPU).  The histogram is 2*ir_len int64 in device memory: [L | R],
 * fixed point with unit e0*2^-frac_bits, so a sum over shards (RCCL int64 SUM) is exact. */
arx_status arx_clear_histogram(arx_renderer* r);
/* Global ray ids, ray_end <= N = x*y*z (the energy and fixed-point normalisation assume N rays). */
arx_status arx_trace_rays(arx_renderer* r, uint64_t ray_begin, uint64_t ray_end);
arx_status arx_histogram_device(arx_renderer* r, int64_t** d_hist, size_t* n_elems);
/* Accumulate into caller-owned device memory (2*ir_len int64, e.g. a torch tensor that RCCL
 * all-reduces in place); NULL restores the renderer's own buffer. */
arx_status arx_attach_histogram(arx_renderer* r, int64_t* d_hist, size_t n_elems);
arx_status arx_finalize_ir(arx_renderer* r);
arx_status arx_ir_device(arx_renderer* r, float** d_left, float** d_right, size_t* ir_len);
arx_status arx_copy_ir(arx_renderer* r, float* h_left, float* h_right, size_t ir_len);
/* Counters of the last frame (synchronises the renderer's stream).  ARX_ERR_INTERNAL (stats still
 * filled in) when the tree as last written has a box off the 16-bit quantization grid (receiver refit
 * or device re-quantization; never with the host's grid bounds). */
arx_status arx_get_stats(arx_renderer* r, arx_stats* out);
/* Device times (HIP events on the renderer's stream) of the last min(n, arx_timing_ring()) trace launches, oldest
 * first, into ms[0..*n_out); synchronises on them.  The reference's timed window (Time taken by
 * Optix, AudioRenderer.cpp:495-518), kept per launch so a benchmark can average a timed region. */
arx_status arx_trace_times(arx_renderer* r, double* ms, size_t n, size_t* n_out);
/* The same for the last min(n, 64) file convolutions (arx_convolute_device / _audio_file; the
 * reference's "Time taken just to convolute", AudioRenderer.cpp:688-696). */
arx_status arx_conv_times(arx_renderer* r, double* ms, size_t n, size_t* n_out);
/* The same for the last min(n, 64) live-path convolutions (arx_convolute_live_* and the streaming
 * convolution's blocks, arx_stream_process*). */
arx_status arx_live_times(arx_renderer* r, double* ms, size_t n, size_t* n_out);
/* Capacity of the per-launch timing rings above (launches kept). */
int32_t arx_timing_ring(void);
/* Per-launch timing on (1, the default) or off (0).  Each timed launch puts two event markers on the
 * stream, ~4.5 us of stream time apiece on MI355X (tools/step_gaps.py): off, trace and file
 * convolution launches go to the stream alone and the rings above stop growing.  A call that asks
 * for its time -- arx_render / arx_group_render with render_ms, arx_convolute_audio_file with
 * convolute_ms -- is timed either way, as the reference times render() only when render_ms is given
 * (AudioRenderer.h:27).  arx_get_stats' trace_ms / conv_ms then report the last timed launch. */
arx_status arx_set_timing(arx_renderer* r, int32_t on);

/* ---- Room-acoustic parameters (ISO 3382-1) of the traced histogram ---------------------------
 * No reference counterpart: the reference only ever convolves its IR.  Per channel c (0 left ear,
 * 1 right ear, 2 left + right: the curve of the mono IR), with h[k] >= 0 the histogram bin in
 * fixed-point units, n = ir_len and sr the sample rate:
 *   E[k] = sum_{j >= k} h[j], k in [0, n], E[n] = 0: Schroeder's decay curve, exact in int64 (so as
 *   independent of the GPU count as the histogram); total = E[0].
 *   onset / last = the first / last bin with h > 0 (-1, -1 when total == 0).
 *   "E[k] is at or below -x dB" means (double)E[k] <= (double)E[0] * Cx, "at or above" >=, with the
 *   four f64 literals below -- part of the contract, so the fit ranges are exact integers.
 *   Fit range [a, b], inclusive.  EDT: a = onset, b = the last bin with E > 0 at or above -10 dB.
 *   T20: a = the first bin >= onset at or below -5 dB, b = the last bin with E > 0 at or above
 *   -25 dB.  T30: as T20 with -35 dB.  A range is valid when b - a >= 1; (a, b) = (-1, -1) when no
 *   such bins exist.
 *   Fit, centred: x_k = k - (a + b)/2, y_k = 10 log10((double)E[k] / (double)E[0]), slope =
 *   sum x_k y_k / sum x_k^2 (dB per bin), T = -60 / (slope * sr) seconds, EDT by the same formula on
 *   its own range.  A time is valid when its range is and slope < 0.
 *   Windows: n50 = (50 sr + 500) / 1000, n80 = (80 sr + 500) / 1000 (integer division);
 *   early50 = E[onset] - E[min(onset + n50, n)], late50 = E[min(onset + n50, n)], both exact;
 *   C50 = 10 log10(early50 / late50), +inf when late50 == 0 and early50 > 0; D50 = early50 / total;
 *   C80 the same with n80.  C50 / D50 (C80) are valid when n50 (n80) > 0 and total > 0, C50 / C80
 *   when early > 0 as well.
 *   Ts = (sum_{k > onset} (k - onset) h[k]) / (total * sr) seconds, the numerator summed in 128 bits
 *   (it passes 64 for histograms the engine can produce) and converted to f64 once.
 *   total == 0: every float NaN, every bin -1, valid == 0 (and the status ARX_OK).  Invalid
 *   quantities are NaN.
 * The analysis describes the last TRACED histogram (or the attached one), never the f32 IR: an IR
 * installed with arx_set_ir is not analysed. */
#define ARX_ACOUSTICS_C5  3.1622776601683794e-01 /* 10^-0.5 */
#define ARX_ACOUSTICS_C10 1.0000000000000001e-01 /* 0.1 */
#define ARX_ACOUSTICS_C25 3.1622776601683794e-03 /* 10^-2.5 */
#define ARX_ACOUSTICS_C35 3.1622776601683794e-04 /* 10^-3.5 */
#define ARX_VALID_EDT 0x01u
#define ARX_VALID_T20 0x02u
#define ARX_VALID_T30 0x04u
#define ARX_VALID_C50 0x08u
#define ARX_VALID_C80 0x10u
#define ARX_VALID_D50 0x20u
#define ARX_VALID_TS  0x40u
typedef struct arx_acoustics {
    int64_t total;              /* E[0], fixed-point units */
    double unit;                /* energy per unit: e0 * 2^-frac_bits (arx_finalize_ir's) */
    double edt_s, t20_s, t30_s; /* seconds */
    double c50_db, c80_db, d50;
    double ts_s;                /* seconds */
    int32_t onset_bin, last_bin;
    int32_t edt_bins[2], t20_bins[2], t30_bins[2]; /* fit ranges [a, b] */
    uint32_t valid;             /* ARX_VALID_* */
    uint32_t reserved;          /* 0: the struct's size is a multiple of 8 with no implicit padding */
} arx_acoustics;
/* Queue the analysis of the last started frame's histogram (the attached one when there is one) on
 * that frame's stream: the decay curves of the three channels, then their parameters.
 * Asynchronous, no host synchronisation (the first analysis of a frame set allocates its buffers).
 * In a group, call it on a member after arx_group_render: the all-reduced histogram is already
 * there.  Needs no scene. */
arx_status arx_analyze_ir(arx_renderer* r);
/* on != 0: arx_render and arx_group_render queue the analysis right after the IR finalize of every
 * frame.  Off by default; off, nothing new is launched and no output changes by a bit. */
arx_status arx_set_auto_analyze(arx_renderer* r, int32_t on);
/* Channel 0 / 1 / 2 of the last started frame's analysis; synchronises that frame's stream, like
 * arx_get_stats.  ARX_ERR_NOT_READY when no analysis was queued for that frame. */
arx_status arx_get_acoustics(arx_renderer* r, int32_t channel, arx_acoustics* out);
/* The decay curves in device memory: 3*ir_len int64, channel 0, then 1, then 2 (NULL before the
 * frame set's first analysis). */
arx_status arx_edc_device(arx_renderer* r, int64_t** d_edc, size_t* n_elems);
/* One channel's curve to the host; synchronising.  ARX_ERR_NOT_READY like arx_get_acoustics. */
arx_status arx_copy_edc(arx_renderer* r, int32_t channel, int64_t* h_edc, size_t ir_len);
/* Device times of the last min(n, arx_timing_ring()) analyses (scan to results), oldest first, like
 * arx_live_times; obeys arx_set_timing. */
arx_status arx_analysis_times(arx_renderer* r, double* ms, size_t n, size_t* n_out);
/* Host only, no device needed: the same definitions in plain C++.  left / right: ir_len bins >= 0
 * whose sum fits int64 (ARX_ERR_INVALID_ARGUMENT otherwise, and for NULL, ir_len == 0 or
 * sample_rate <= 0); out[c] = channel c. */
arx_status arx_acoustics_from_histogram(const int64_t* left, const int64_t* right, size_t ir_len,
                                        int32_t sample_rate, double unit, arx_acoustics out[3]);
/* host only: the log10 the analysis takes for its levels on the device and on the host alike -- IEEE f64 add, mul
 * and div in a fixed order, within 2 ulp, so that the same decay curve gives the same bytes on both sides (libm's
 * and the device library's log10 are not the same function).  out[i] for n arguments; an argument that is not a
 * positive normal number goes to the C library's log10. */
arx_status arx_debug_log10_shared(const double* x, size_t n, double* out);
arx_status arx_edc_from_histogram(const int64_t* hist, size_t ir_len, int64_t* edc);
/* The decay curve's scan kernels: 0 = the product's choice, 1 = one workgroup per channel (one
 * launch), 2 = tiled (tile sums, then an apply that adds up the sums above its tile: two launches;
 * the product's).  Both give the same bits; the first is kept as a measured alternative
 * (tools/acoustics_time.py). */
arx_status arx_debug_set_scan_shape(arx_renderer* r, int32_t shape);

/* Identity of the trace kernel compiled into this library: a hash of its sources and experiment
 * macros (build.py trace_source_id).  Stored PMC profiles carry it with the tree hash and VGPR
 * count, and bench.py uses a stored profile only when all three match its own run.  No
 * reference counterpart (measurement plumbing). */
uint64_t arx_trace_kernel_id(void);
/* The same for the file convolution's kernels (build.py conv_source_id: the kernel headers
 * arx_conv_fft.hpp and arx_conv_kernels.hpp, not the host code that launches them): the guard of
 * the stored convolution traffic profile (profiles/<round>/conv_traffic.json). */
uint64_t arx_conv_kernel_id(void);
/* Replace the renderer's IR with caller data (host, ir_len floats per ear), e.g. a stored or
 * measured IR; the next convolution uses it.  No reference equivalent (its IR only comes
 * from render()). */
arx_status arx_set_ir(arx_renderer* r, const float* h_left, const float* h_right, size_t ir_len);
/* Same from device memory on the renderer's device (e.g. another renderer's IR, arx_ir_device),
 * asynchronous on the renderer's stream: the caller orders it after the IR's producer (a HIP
 * event) and keeps the source unchanged until the copy has run. */
arx_status arx_set_ir_device(arx_renderer* r, const float* d_left, const float* d_right, size_t ir_len);
int arx_frac_bits(uint64_t n_rays_total);

/* ---- Multi-GPU ray sharding ------------------------------------------------------------------
 * No reference equivalent: the reference renders on device 0 only (AudioRenderer.cpp:252) and has
 * no collective (SURVEY.md §2, §8b "set device count", §8e).  A group holds one renderer per GPU;
 * rank g of G traces the global ray ids [g*N/G, (g+1)*N/G) of the same N = x*y*z ray launch, and
 * ONE RCCL all-reduce (int64 SUM over xGMI) of the 2*ir_len fixed-point histogram leaves the full
 * IR on every member -- exact, so the IR is bitwise independent of G.  Convolution then runs on any
 * member (arx_group_member + arx_convolute_*). */
typedef struct arx_group arx_group;
/* One process driving n_devices GPUs: devices[i] (devices NULL = 0..n_devices-1), ncclCommInitAll
 * (also for n_devices = 1).  cfg->device is ignored.  Listing ONE device several times
 * oversubscribes it (e.g. to run the sharded path on a single-GPU box): RCCL cannot take a device
 * twice, so such a group sums its shards on that device instead (the same exact int64 sum). */
arx_status arx_group_create(const arx_config* cfg, const int32_t* devices, int32_t n_devices, arx_group** out);
/* One GPU per process (torchrun-style launch): rank 0 calls arx_group_unique_id and shares the
 * ARX_GROUP_ID_BYTES bytes out of band; every rank then calls arx_group_create_rank with its rank and
 * cfg->device (ncclCommInitRank).  id may be NULL when n_ranks == 1. */
#define ARX_GROUP_ID_BYTES 128
arx_status arx_group_unique_id(uint8_t* id, size_t id_bytes);
arx_status arx_group_create_rank(const arx_config* cfg, int32_t n_ranks, int32_t rank, const uint8_t* id,
                                 size_t id_bytes, arx_group** out);
void arx_group_destroy(arx_group* g);
int32_t arx_group_members(const arx_group* g); /* renderers in this process */
int32_t arx_group_ranks(const arx_group* g);   /* G: shards of the launch */
/* Member i's renderer (owned by the group; NULL if out of range) for convolution / IR access. */
arx_renderer* arx_group_member(arx_group* g, int32_t i);
/* The scene tree is built ONCE per group on the host and shared by every member (each uploads it
 * to its own device); in a one-GPU-per-process group (arx_group_create_rank) this is collective:
 * rank 0 builds and the tree goes to the other ranks with one RCCL broadcast over xGMI, so every
 * rank must call it (their arrays are not read). */
arx_status arx_group_set_scene(arx_group* g, const float* tri_vertices, const float* tri_absorption, int64_t n_tris);
/* The shard of rank `rank` of `n_ranks` in an n-ray launch: global ray ids [begin, end) =
 * [rank*n/n_ranks, (rank+1)*n/n_ranks) (exact 128-bit products).  Host only; arx_group_render uses it. */
void arx_group_shard(uint64_t n_rays, int32_t rank, int32_t n_ranks, uint64_t* begin, uint64_t* end);
/* Tests only: arx_group_set_scene's one-GPU-per-process hand-over (rank 0 checks and builds the
 * scene, the other ranks read its broadcast byte image; a failure on any rank fails the call on all)
 * over a caller's transport instead of RCCL.  word(ctx, v, op): op 0 = broadcast *v from rank 0,
 * op 1 = all-reduce max into *v; bytes(ctx, buf, n): broadcast n bytes from rank 0's buf into every
 * rank's; both collective, 0 on success.  Host only; tree_hash = the tree every rank now holds. */
typedef int (*arx_share_u64_fn)(void* ctx, uint64_t* value, int op);
typedef int (*arx_share_bytes_fn)(void* ctx, uint8_t* buf, uint64_t n);
arx_status arx_debug_share_scene(int32_t rank, const float* tri_vertices, const float* tri_absorption, int64_t n_tris,
                                 arx_share_u64_fn word, arx_share_bytes_fn bytes, void* ctx, uint64_t* tree_hash);
/* The single-renderer setters, applied to every member. */
arx_status arx_group_set_receiver_model(arx_group* g, int side, const float* tri_vertices_local, int64_t n_tris);
arx_status arx_group_set_emitter(arx_group* g, float x, float y, float z);
arx_status arx_group_set_listener(arx_group* g, float x, float y, float z, float yaw_deg);
arx_status arx_group_set_thresholds(arx_group* g, float energy, uint32_t max_bounces);
arx_status arx_group_set_hrtf_absorption_rate(arx_group* g, float rate);
arx_status arx_group_set_base_power(arx_group* g, float base_power);
arx_status arx_group_set_mono_output(arx_group* g, int mono);
arx_status arx_group_set_seed(arx_group* g, uint64_t seed);
/* render() over the group: clear, trace every local shard, all-reduce, finalize on every member
 * (async on the members' streams).  render_ms (if not NULL; synchronises) = the longest shard's
 * trace kernel time.  After an error the members may be at different frames (and, on the rank path,
 * peers may wait in the collective this rank skipped): destroy the group, do not render on it again. */
arx_status arx_group_render(arx_group* g, double* render_ms);
/* arx_set_frames_in_flight on every member; a member's all-reduce waits for its previous one, so
 * the collectives on each communicator keep their order.  That event chain runs on one GPU with
 * every collective forced (arx_debug_group_force_collectives, tests/test_gpu_collectives.py: 1 to 3
 * frames, in and out of place, bit-identical to a plain renderer); its first multi-GPU run is the
 * 8-GPU bench, which keeps the one-GPU frames-in-flight policy at every N. */
arx_status arx_group_set_frames_in_flight(arx_group* g, int32_t n);
/* arx_set_timing on every member; with it on (or render_ms asked for), arx_group_render also puts HIP
 * events around each member's histogram all-reduce. */
arx_status arx_group_set_timing(arx_group* g, int32_t on);
/* Device times of member `member`'s last min(n, 256) timed histogram all-reduces (the RCCL collective's
 * window on that member's stream, queueing behind the member's own trace excluded), oldest first;
 * synchronises on them.  *n_out = 0 when no all-reduce was timed (a one-rank group skips its no-op
 * all-reduce unless arx_debug_group_force_collectives). */
arx_status arx_group_allreduce_times(arx_group* g, int32_t member, double* ms, size_t n, size_t* n_out);

/* Time-block sharded file convolution ("time blocks sharded ... only the n - sr overlap
 * is summed at shard seams"; the reference convolves on one GPU, kernels.cu:404-430).  The file's
 * floor(n/sr) one-second blocks form P = ceil(blocks / 2) FFT pairs; rank g of G convolves the pairs
 * [g*P/G, (g+1)*P/G) with its member's IR and writes the output frames they own,
 * arx_group_conv_shard's [begin, end), into its member's full-length buffers d_out_left[i] /
 * d_out_right[i] (n_frames floats each, on member i's device; d_in[i] there holds the whole file).
 * The seam -- the tail of the block before a shard -- is re-made by the shard itself from that block's
 * input, not received from the neighbour, so the data path has no collective; the union of the ranks'
 * frames is arx_convolute_device's output bit for bit.  Plans without the chained pass
 * (arx_group_conv_sharded == 0: ir_len != 2 sr, or an IR length without a direct mixed-radix split)
 * convolve and write the whole file on every rank.  Asynchronous on the members' streams, like
 * arx_convolute_device; arx_conv_times per member time each shard. */
arx_status arx_group_convolute_device(arx_group* g, const float* const* d_in, size_t n_frames,
                                      float* const* d_out_left, float* const* d_out_right);
/* AudioRenderer::convoluteAudioFile over the group (AudioRenderer.cpp:663-750: host buffers, sizes in
 * BYTES, reference normalisation): every member of this process convolves its time-block shard
 * (arx_group_convolute_device), copying in only the input its pairs read and copying back only the
 * frames it owns, so in a group of one process over several GPUs h_out_left / h_out_right receive
 * the whole convolved file -- bit-identical to arx_convolute_audio_file -- with the work spread over
 * the GPUs.  On the one-GPU-per-process path each process fills its own ranks' frames (the caller
 * gathers).  One rank, or a plan that does not shard: arx_convolute_audio_file on member 0.
 * convolute_ms = the longest member's convolution window, process_ms = the longest member's whole
 * call window (copies included); synchronising. */
arx_status arx_group_convolute_audio_file(arx_group* g, const float* h_in, size_t in_bytes, float* h_out_left,
                                          float* h_out_right, double* convolute_ms, double* process_ms);
/* The output frames [begin, end) rank `rank` of n_ranks owns in a sharded convolution of n_frames at
 * sample_rate (host only; ranges of the ranks tile [0, n_frames)). */
void arx_group_conv_shard(int32_t sample_rate, uint64_t n_frames, int32_t rank, int32_t n_ranks, uint64_t* begin,
                          uint64_t* end);
/* 1 if the group's convolution plan shards (see arx_group_convolute_device), 0 if every rank convolves
 * the whole file, -1 on error. */
int32_t arx_group_conv_sharded(arx_group* g);
arx_status arx_group_synchronize(arx_group* g);
arx_status arx_group_copy_ir(arx_group* g, float* h_left, float* h_right, size_t ir_len); /* member 0 */
/* Queries / receiver hits / misses summed over this process's members; times = the longest. */
arx_status arx_group_get_stats(arx_group* g, arx_stats* out);
/* values[0..n) of this process combined over all processes of the group (op 0 = sum, 1 = max)
 * with one RCCL all-reduce, in place; synchronising, so it doubles as a barrier.  A group whose
 * members all live in this process returns values unchanged. */
arx_status arx_group_allreduce_f64(arx_group* g, double* values, size_t n, int op);

/* AudioRenderer::convoluteAudioFile (AudioRenderer.h:31; AudioRenderer.cpp:663-750) over
 * convoluteFromAudioBuffer (kernels.cuh:21; kernels.cu:382-438): 1-s blocks zero padded to
 * ir_len, circular convolution with each IR, overlap-added, tail (len mod sr) unprocessed,
 * divided by (ir_len/2).  Host buffers, sizes in BYTES like the reference. */
arx_status arx_convolute_audio_file(arx_renderer* r, const float* h_in, size_t in_bytes, float* h_out_left,
                                    float* h_out_right, double* convolute_ms, double* process_ms);
/* Same on device-resident buffers (n_frames floats each); no host synchronisation. */
arx_status arx_convolute_device(arx_renderer* r, const float* d_in, size_t n_frames, float* d_out_left,
                                float* d_out_right);
/* Input reuse for the reference's re-render pattern: full_render_cycle (AudioRenderer.cpp:790-798,
 * called by main.cpp:40-67 on every listener move) convolves the SAME file with every new IR.
 * arx_convolute_prepare_input transforms the file's one-second blocks once (device input, n_frames
 * samples).  The transform is queued on the renderer's stream, not run by the call: the caller may
 * overwrite d_in only once that stream has finished it (after arx_get_stats, arx_copy_ir or a
 * synchronisation of the stream, or from work ordered after it on that stream); arx_convolute_prepared then
 * convolves them with the renderer's current IR into the caller's device outputs (n_frames each,
 * *n_frames set when non-NULL) -- bit-identical to arx_convolute_device on the same input, without
 * the input's forward transform.  The prepared input stays until the next arx_convolute_device /
 * arx_convolute_audio_file / arx_convolute_prepare_input on this renderer (ARX_ERR_NOT_READY after). */
arx_status arx_convolute_prepare_input(arx_renderer* r, const float* d_in, size_t n_frames);
arx_status arx_convolute_prepared(arx_renderer* r, float* d_out_left, float* d_out_right, size_t* n_frames);

/* AudioRenderer::convoluteLiveInput (AudioRenderer.h:29; AudioRenderer.cpp:593-661) over
 * convoluteFromLiveInput (kernels.cu:345-377) minus the CircularBuffer (which stays with the
 * caller, include/arx_circular_buffer.hpp): one mic block of in_bytes/8 f64 samples (<= ir_len),
 * zero padded to ir_len, circularly convolved with each IR in f64, divided by (ir_len/2) and
 * zipped L/R into h_out[2*ir_len] (out_len must be 2*ir_len).  IR spectra are cached between
 * callbacks (the reference re-plans and re-transforms them every callback). */
arx_status arx_convolute_live_block(arx_renderer* r, const double* h_in, size_t in_bytes, double* h_out,
                                    size_t out_len);
/* Same on device buffers (n_in f64 samples in, 2*ir_len f64 out), no host synchronisation. */
arx_status arx_convolute_live_device(arx_renderer* r, const double* d_in, size_t n_in, double* d_out);
/* Recompute the cached IR spectra now (async on the renderer's stream) instead of lazily in the
 * next convolution: which = 1 file path, 2 live path, 3 both.  Lets a moving-listener frame
 * (re-trace + reduce + new spectra) finish before audio needs it. */
arx_status arx_prepare_ir_spectra(arx_renderer* r, int which);
/* Describe the convolution plan (which = 1 file path, 2 live path; created if needed) into
 * buf[len]: "mixed-radix direct circular: n=.. sr=.. (N1xN2) f64" when ir_len factors into two
 * 7-smooth sub-lengths <= 512 (FFT length = ir_len, as the reference's cuFFT plans), else
 * "pow2 linear+fold: ..." (power-of-two length >= ir_len + block - 1, folded back). */
arx_status arx_conv_describe(arx_renderer* r, int which, char* buf, size_t len);

/* Streaming convolution for the RtAudio duplex callback (replaces the
 * per-callback full-length circular convolution of convoluteLiveInput, AudioRenderer.cpp:593-661,
 * whose 2*ir_len outputs the reference's CircularBuffer wraps onto itself, main.cpp:189-195, which
 * stays available as arx_convolute_live_block -- the compat path).  Uniformly partitioned
 * overlap-save in f64 on the renderer's device and stream: each call consumes one block of
 * n_frames <= block_frames f64 input frames (shorter blocks are zero padded) and returns
 * block_frames output frames zipped L/R (2*block_frames doubles) = the linear convolution of the
 * input stream with the renderer's current IR, scaled like the reference's live path
 * (ir_len / (ir_len/2), normalizeBuffers).  Latency: one block.  A new IR (render, set_ir) applies
 * from the next block on; the input history is kept, so the stream does not restart -- but without
 * a crossfade (below; off by default) the output steps from x * h_old to x * h_new within one
 * sample at that block boundary.  block_frames in [1, min(4096, ir_len)]. */
typedef struct arx_stream arx_stream;
arx_status arx_stream_create(arx_renderer* r, int32_t block_frames, arx_stream** out);
void arx_stream_destroy(arx_stream* s);
arx_status arx_stream_reset(arx_stream* s); /* forget the input history */
arx_status arx_stream_info(const arx_stream* s, int32_t* block_frames, int32_t* partitions, int32_t* fft_size);
arx_status arx_stream_process(arx_stream* s, const double* h_in, size_t n_frames, double* h_out, size_t out_len);
/* Same on device buffers (n_frames f64 in, 2*block_frames f64 out), no host synchronisation. */
arx_status arx_stream_process_device(arx_stream* s, const double* d_in, size_t n_frames, double* d_out);

/* Crossfade at an IR change.  The stream keeps two sets of partition spectra: the current one and,
 * once a fade was enabled, the one the previous block used (allocated by the first call that
 * enables a fade, the size of the first: 3 MB at 48 kHz x 2 s x 4096 frames;
 * ARX_ERR_OUT_OF_MEMORY if that fails).  A block is a transition block when fade_frames > 0, the
 * renderer's IR generation differs from the one the current spectra were made from, and the stream
 * has processed at least one block since it was created or last reset.  On a transition block the
 * two sets are swapped, the new current set is built, both outputs are computed from the same
 * delay line (this block's input included), and per ear
 *     out[i] = fma(w[i], y_new[i] - y_old[i], y_old[i])  for frames i < fade_frames,
 *     out[i] = y_new[i]                                  after,
 * both y already scaled.  The first block of a stream and the first block after arx_stream_reset
 * are never transition blocks: they use the current IR only.  Several IR changes between two
 * blocks count as one (the old set is whatever the previous block used); an IR change before each
 * of two consecutive blocks makes two consecutive transition blocks, each from the previous
 * block's IR to its own.  With fade_frames == 0 the stream runs the kernels it always ran, to the
 * same bits; with a fade enabled every block that is no transition does too, and so does a
 * transition between two IRs with the same samples (arx_set_ir with the same data bumps the
 * generation).  Nothing here adds a host or device synchronisation to arx_stream_process*: the
 * weight table is uploaded by arx_stream_set_crossfade, ordered on the renderer's stream like
 * arx_stream_reset, and holds exactly arx_stream_fade_weights' values.  Fades longer than a block
 * and fades on the compat path (arx_convolute_live_block) are not provided. */
#define ARX_FADE_LINEAR 0
#define ARX_FADE_HANN   1
/* Host only.  w[0..fade_frames) = the weight of the NEW IR's output on frame i of a transition block:
 * t = (i + 0.5) / fade_frames;  LINEAR: w = t;  HANN: w = 0.5 - 0.5 cos(pi t).  Complementary
 * (w[i] + w[F-1-i] == 1 to rounding), strictly inside (0, 1), increasing. */
arx_status arx_stream_fade_weights(int32_t shape, int32_t fade_frames, double* w);
/* fade_frames in [0, block_frames]; 0 (the default) = the hard switch. */
arx_status arx_stream_set_crossfade(arx_stream* s, int32_t fade_frames, int32_t shape);
arx_status arx_stream_get_crossfade(const arx_stream* s, int32_t* fade_frames, int32_t* shape);
/* Transition blocks processed since the stream was created. */
arx_status arx_stream_crossfades(const arx_stream* s, uint64_t* n);

/* Tests only: issue every collective of the group even at one rank -- the histogram all-reduce of
 * arx_group_render (with frames in flight on every member's frame stream, chained by events), the
 * f64 all-reduce of arx_group_allreduce_f64 and the rank path's scene broadcast of
 * arx_group_set_scene -- so a one-GPU box runs the RCCL call paths a multi-GPU job takes.  out_of_place
 * != 0: the all-reduces write separate receive buffers pre-filled with 0xFF (the histogram's is then
 * copied back), so the result is right only if the collective moved the data.  Synchronises the
 * members first.  ARX_ERR_INVALID_ARGUMENT for a group without a communicator (one GPU listed
 * several times). */
arx_status arx_debug_group_force_collectives(arx_group* g, int32_t on, int32_t out_of_place);
/* Collectives the group has issued: out3[0] histogram all-reduces, [1] f64 all-reduces, [2] scene
 * broadcasts (rank path). */
arx_status arx_debug_group_collectives(const arx_group* g, uint64_t* out3);

/* The ray direction buffer across launches, and the order the ray pool hands rays out in.
 *
 * A ray's direction is a pure function of (seed, ray id), so each frame set keeps the float4
 * directions its last trace launch used and the next launch re-makes them only when the seed, the
 * first ray or the ray count differ, when the buffer had to grow (a larger launch reallocates it
 * and forgets its content), or when arx_set_stream named another stream since.  Nothing else invalidates the directions: not the scene, the emitter, the
 * listener or the thresholds.
 *
 * Launches large enough for the ray pool (arx_stats.trace_grid_cus; 16-bit nodes, LDS stack) also
 * order the pool's part of the buffer longest ray first: the first such launch of a key runs a
 * measuring instance of the trace kernel (same rays, arithmetic and results; it also stores each
 * ray's node + leaf steps, and the largest count for a ray that ended on the receiver: its length
 * changes with the listener, so it starts first), a device counting sort by descending cost follows
 * on the same stream, and the launches after it hand out the sorted buffer for as long as the key
 * holds.  The key is all that
 * moves a ray's path: the scene (every arx_set_scene, and the tree hash), emitter, seed, ray range,
 * max_bounces, energy threshold, IR length (distance limit), base power and ray count (initial
 * energy), hrtf_absorption_rate, is_mono, the kernel instance and the pool's share.  The listener's
 * position and yaw are not in it.  A changed key measures and sorts again.  The int64 histogram and
 * the counters do not depend on the order rays run in, so every mode gives the same bits.
 *
 * mode 0: directions kept, always in ray order (no measuring, no sort);
 * mode 1: the above;
 * mode 2: directions re-made by every launch, in ray order (nothing kept).
 * Takes effect at the next trace launch of each frame set. */
arx_status arx_debug_set_ray_order(arx_renderer* r, int32_t mode);
/* Tests only (synchronises): the first `count` float4 slots (x, y, z, 0) of the current frame set's
 * direction buffer as its last launch left it, the ray id of slot 0 in ray order, the number of
 * leading slots still in ray order (the static ranges; all of them when the buffer is not sorted) and
 * whether the pool's slots are sorted. */
arx_status arx_debug_ray_order_buffer(arx_renderer* r, float* h_out_xyzw, uint64_t count, uint64_t* first_ray,
                                      uint64_t* n_static, int32_t* sorted);
/* Host only: the helpers the trace kernel and the pool's sort share -- the statically dealt rays of a
 * launch of n with dyn_share / 256 of them in the pool, a step count as the measuring instance stores
 * it (saturated to 16 bits), and this build's dyn_share.  Any output may be NULL. */
arx_status arx_debug_ray_order_host(uint64_t n, uint32_t dyn_share, uint32_t steps, uint64_t* n_static, uint32_t* cost16,
                                    uint32_t* build_share);

/* The path cache: a repeated key answers its queries from the scene-only hits of an earlier launch.
 *
 * A ray's path through the static scene does not depend on the listener: the receiver enters a query
 * only as one more candidate for the closest hit (the lexicographic minimum of (t, triangle id), so
 * the order candidates are tested in does not matter), and a receiver hit ends the ray.  The renderer
 * therefore keeps, for one key, the scene-only closest hit of every query of every ray (24 B each,
 * laid out [bounce][slot]) with its own copy of the direction buffer they were recorded on, and a
 * frame of that key is one plain kernel: per query the cached hit, a closest-hit query over the
 * receiver sub-tree alone that starts from it, and the same shading.  Histogram, IR and the queries /
 * receiver_hits / misses counters are bit for bit those of the full traversal.
 *
 * The key is the ray order's (arx_debug_set_ray_order) without the kernel instance and the pool's
 * share, and holds for every launch on 16-bit nodes and the LDS stack, ray pool or small: scene (every
 * arx_set_scene, and the tree hash), emitter, seed, ray range, max_bounces, energy threshold, distance
 * limit, initial energy, hrtf_absorption_rate, is_mono.  The listener and the receiver model are not
 * in it.
 *   - The first launch of a key is traced exactly as without the cache (and costs what it did).
 *   - The first launch whose key equals the previous launch's, on a direction buffer this launch
 *     neither fills nor measures, records (one scene-only pass of the trace kernel's recording
 *     instance into the cache) and then replays: about one trace plus one replay.
 *   - Later launches of the key only replay.  So a caller whose emitter or scene changes every frame
 *     never records; one that moves only the listener pays two traced-cost launches (three with two
 *     frames in flight: each set measures its own buffer first), then replays.
 * Any key change returns to "traced" and drops the records.  Never cached, traced as before: the
 * global stack, CW4 and f32-node paths, a caller's own stream (arx_set_stream), and launches whose
 * records (max_bounces x rays x 24 B, plus 16 B per ray of directions; 384 MB at 1M rays x 16) exceed
 * max_bytes (default 1 GiB) or do not fit on the device (reported as over the cap and not tried
 * again until this call).  A scene's own receiver-marked triangles (absorption -1 / -2) are cached
 * like any other: the recording ends a ray on them without a histogram, the replay adds their energy.
 * The buffer is allocated at the first recording, kept across keys, and freed when it must grow and
 * at arx_destroy.  arx_trace_times' window of a launch covers whatever ran
 * for it; arx_stats' trace_* fields keep describing the traced instance the launch's arguments take.
 * Throughput figures derived from arx_stats.queries count replayed queries like traced ones.
 *
 * mode 0: off (every launch traced); mode 1 (default): the above.  Either call drops the records. */
arx_status arx_debug_set_path_cache(arx_renderer* r, int32_t mode, uint64_t max_bytes);
#define ARX_PATH_OFF 0
#define ARX_PATH_TRACED 1
#define ARX_PATH_RECORDED 2      /* recorded by the last launch (which also replayed) */
#define ARX_PATH_REPLAYED 3
#define ARX_PATH_NOT_CACHEABLE 4
#define ARX_PATH_OVER_CAP 5
/* What the last trace launch did (ARX_PATH_*), the bytes of records held (0 without a recording) and
 * the queries the recording ran (synchronises when asked for).  Any output may be NULL. */
arx_status arx_debug_path_cache_state(arx_renderer* r, int32_t* state, uint64_t* bytes, uint64_t* queries_recorded);
/* Host only: bytes of records for n_rays x max_bounces queries. */
uint64_t arx_debug_path_cache_bytes(uint64_t n_rays, uint32_t max_bounces);

/* The path filter: a replayed frame runs only the queries whose segment crosses the receiver's box.
 *
 * Nothing a query starts from (position, direction, energy, distance so far) depends on the listener
 * either, so with the filter on (the default) the recording launch stores that as well: 32 B per query
 * and 16 + 2 B per ray beside the 24-B records.  A replayed frame is then two launches.  The first reads
 * each ray's stored positions once (16 B per query) and tests every segment against the receiver's
 * box, grown by 2^-7 m plus rounding slack, as the receiver refit left it on the device.  A ray none of
 * whose segments meets the box adds its recorded query count and is done; the others -- with every
 * ray whose last query missed or ended on a receiver-marked triangle of the scene -- are listed, and
 * the second launch replays their candidate queries alone, each from its stored state with the
 * unfiltered replay's functions on the same bits.  Results are bit for bit the unfiltered replay's.
 *
 * This memory is OUTSIDE arx_debug_set_path_cache's max_bytes, which keeps counting the 24-B records
 * alone: rays x (32 x max_bounces + 18) B of planes per renderer, plus 16 x rays B of candidate list
 * and 16 B per 1024 rays of list heads per frame set that replays (at 1M rays x 16 bounces: 530 MB of planes and 16 MB per list,
 * so 546 MB with one frame in flight and 562 MB with two).
 * If it does not fit on the device the launch records and replays unfiltered, and that size is not
 * tried again until the filter is switched off and on.  Also unfiltered, exactly as before: launches
 * with max_bounces > 64, and frames whose emitter lies inside the receiver's grown box (every ray
 * would be a candidate).  Switching the filter on over records made without state forgets them: the
 * key's next launch records again, once (state "recorded"); switching it off keeps them. */
arx_status arx_debug_set_path_filter(arx_renderer* r, int32_t on);
/* Whether the last trace launch was a filtered replay, the bytes held for the filter (planes and
 * lists), and that launch's candidate rays and candidate queries (0 unless filtered; synchronises
 * when either is asked for).  Any output may be NULL. */
arx_status arx_debug_path_filter_state(arx_renderer* r, int32_t* filtered, uint64_t* bytes, uint64_t* candidate_rays,
                                       uint64_t* candidate_queries);
/* Host only: bytes of the filter's planes for n_rays x max_bounces queries plus n_lists candidate lists. */
uint64_t arx_debug_path_filter_bytes(uint64_t n_rays, uint32_t max_bounces, uint32_t n_lists);

/* A batch of listeners rendered from one recorded path set in one call.
 *
 * Neither the path cache's records nor the path filter's planes depend on the listener, so a listener is
 * only a question asked of stored data.  arx_render_listeners answers n of them:
 *
 *   saved = listener; for j in 0..n-1: arx_set_listener(poses[j]); arx_render(); [arx_analyze_ir()];
 *   collect j;  arx_set_listener(saved)
 *
 * and its outputs are bit for bit that loop's: ir_left / ir_right the finalized f32 IRs (n x ir_len each,
 * merged as arx_render merges them with is_mono; host or device memory, copied with hipMemcpyDefault on
 * the renderer's stream like arx_memcpy; both NULL: no IR copies), acoustics arx_get_acoustics' structs
 * (n x 3: channel 0, 1, 2 per listener; host memory; NULL: no analysis), results arx_get_stats' three
 * counters per listener (host memory; NULL: none), *ms the device time of the whole call (a pair of
 * events; recorded when ms is given or arx_set_timing is on).  Afterwards "the last frame" of every
 * getter (arx_copy_ir, arx_get_stats, arx_histogram_device, arx_get_acoustics when acoustics was given,
 * the IR generation streams follow) is pose n-1's, the listener is the one set before the call, and the
 * path cache's records stay.  The per-launch timing ring (arx_trace_times) is advanced only by the poses
 * that take the one-listener route.  n == 0: ARX_OK, nothing is touched.  The call synchronises once, at
 * its end.
 *
 * ARX_ERR_INVALID_ARGUMENT: NULL r, NULL poses with n > 0, exactly one IR pointer NULL, a non-finite
 * pose, more than one frame in flight, a caller's own stream (arx_set_stream), an attached histogram.
 * ARX_ERR_NOT_READY without a scene.
 *
 * Routing.  While the cache holds no recording with filter state for the current key, the next pose runs
 * through arx_set_listener + arx_render proper (the cache's usual warm-up: the key's first launch is
 * traced, its second records and replays) and reports ARX_LISTENER_SINGLE.  Once it does, the remaining
 * poses are answered in chunks by batched kernels: per chunk one clear, one receiver refit that places
 * every listener's receiver into a slot of its own behind the renderer's receiver in the node and
 * triangle arrays, one filter pass in which one read of the stored segments is tested against eight
 * listeners' boxes, one candidate launch for the whole chunk, then the finalizes, analyses and copies.
 * Where that state never comes (cache off, not cacheable or over its cap; filter off or without room;
 * max_bounces > 64; a receiver too large for the device refit; no room for the scratch) every pose takes
 * the one-listener route; a single pose takes it in place when the emitter lies inside its grown
 * receiver box or its receiver cannot be put on the quantization grid.  So the call works wherever
 * arx_render works; the batched kernels show only in `route` and on the clock.  Before the first chunk
 * the quantization grid is grown, once, to hold the remaining poses' receivers, as a walking listener
 * grows it; results do not depend on the grid.  A slot refit that leaves the grid ends the call with
 * ARX_ERR_INTERNAL.
 *
 * Memory, OUTSIDE arx_debug_set_path_cache's max_bytes like the filter's planes: one scratch allocation
 * per renderer, made by the first batched call, kept across calls, freed when it must grow and at
 * arx_destroy.  Per listener of a chunk (arx_debug_listener_bytes):
 *   96 x recv_nodes + 48 x recv_tris   its receiver slot (64-B and 32-B nodes, 48-B triangle records)
 *   + 96 + 112                         its top node and its table entry
 *   + 16 x ir_len + 128 + 336          histogram, counter block, three arx_acoustics
 *   + 8 x ir_len                       its f32 IR pair
 *   + 16 x rays + 16 x ceil(rays/1024) its candidate list and the list's heads
 *   + 16 + 64 x ceil(rays/1024)        the candidate launch's work items
 * (the slots live in the node and triangle arrays, which the first batched call widens), plus, whatever
 * the chunk, one decay-curve buffer of 24 x ir_len B and the analysis kernels' scratch.  The automatic
 * chunk is the largest count, at most 64, that keeps this within 512 MiB: at 1M rays, a 2-s IR at 48 kHz
 * and the 1 020-triangle head, 18.5 MB per listener, so 28 listeners (495 MiB; 29 would be 512.5 MiB).
 *
 * Not offered here: groups (no arx_group_render_listeners), the C++ shim, app.py modes and frames in
 * flight.  Turning the IR set into audio -- a signal convolved with a per-block schedule over these IRs,
 * crossfaded at every change -- is arx_convolute_walk (below), which takes ir_left / ir_right as this
 * call wrote them. */
typedef struct arx_listener_pose { float x, y, z, yaw_deg; } arx_listener_pose;          /* 16 B */
#define ARX_LISTENER_BATCHED 0   /* answered by the batched kernels */
#define ARX_LISTENER_SINGLE  1   /* went through the one-listener route (arx_set_listener + arx_render) */
typedef struct arx_listener_result {                                                     /* 48 B, no implicit padding */
    uint64_t queries, receiver_hits, misses;   /* arx_stats' three counters for this listener's frame */
    uint64_t candidate_rays;                   /* batched route only, else 0 */
    int32_t route;                             /* ARX_LISTENER_* */
    int32_t reserved;                          /* 0 */
    uint64_t reserved2;                        /* 0 */
} arx_listener_result;
arx_status arx_render_listeners(arx_renderer* r, const arx_listener_pose* poses, size_t n,
                                float* ir_left, float* ir_right,      /* n*ir_len each, or both NULL */
                                arx_acoustics* acoustics,             /* n*3 (channel 0, 1, 2 per listener), or NULL */
                                arx_listener_result* results,         /* n, or NULL */
                                double* ms);                          /* device time of the whole call, or NULL */
/* listeners per chunk: 0 = automatic (the largest count whose scratch fits the budget), else forced, 1..64 */
arx_status arx_debug_set_listener_chunk(arx_renderer* r, int32_t listeners);
/* host only: scratch bytes of a chunk (slots, tops, per-listener table, histograms, counters, results, IRs,
 * lists, heads): `listeners` times the per-listener sum above */
uint64_t arx_debug_listener_bytes(uint64_t n_rays, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris, int32_t listeners);
/* host only: where chunk slot j lives -- node range, triangle range and top-node index -- for a scene of
 * n_scene_nodes / n_scene_tris and a receiver of recv_nodes / recv_tris: out5 = {node begin, node end,
 * triangle begin, triangle end, top}.  The tree is node 0, the scene's nodes, the renderer's own receiver;
 * the chunk's tops follow at or above the kernels' LDS node cache, then the slots' nodes; the slots'
 * triangles follow the renderer's own.  ARX_ERR_INVALID_ARGUMENT when any range would pass
 * arx_debug_check_tree_limits' limits */
arx_status arx_debug_listener_layout(int64_t n_scene_nodes, int64_t n_scene_tris, int64_t recv_nodes, int64_t recv_tris,
                                     int32_t listeners, int32_t slot, int64_t out5[5]);

/* Frequency-band absorption: every band's frame from one recorded path set, in one call.
 *
 * Real materials absorb differently per octave band, and ISO 3382-1 reports its parameters per band.  A
 * band is the scene with another absorption per triangle.  A specular ray's geometry does not depend on
 * absorption, which enters a frame only as e = e * (1 - ab) at every reflection and through when
 * e > energy_thres stops the ray; and the path cache keeps the scene-only closest hit of every query of
 * every ray.  So one kernel walks each ray's records once, runs the receiver query once per bounce and
 * carries one energy per band into that band's own histogram: all bands for about the price of one
 * unfiltered replayed frame, with no scene build per band.
 *
 * Contract: band b's outputs are bit for bit those of a renderer whose scene is the same triangles with
 * table[b] as absorption, every other setting and the listener equal, after arx_render and arx_analyze_ir:
 * both finalized IR channels (merged as arx_render merges them with is_mono), the three counters and the
 * three arx_acoustics.
 *
 * The rule for the table (arx_band_table_check; arx_set_band_absorption checks it against the absorption
 * the scene's triangle records carry): for every scene triangle t and band b, table[b * n_tris + t] >=
 * the scene's absorption of t, and every value lies in [0, 1]; a triangle the scene marks -1 or -2 (its own
 * receiver halves) carries the same mark in every band.  Then a band's energy never exceeds the recorded
 * ray's at the same bounce (f32 1 - ab and the product by a non-negative e are monotone under rounding), so
 * every query a band runs has a record.  A scene whose absorption is the minimum over its bands always
 * satisfies it.  A violation, a NaN included, is ARX_ERR_INVALID_ARGUMENT and arx_last_error() names the
 * band and the triangle; so are n_tris other than the scene's and n_bands outside [0, ARX_MAX_BANDS].
 * n_bands 0 drops the table, and so does every arx_set_scene.  A call that fails with
 * ARX_ERR_INVALID_ARGUMENT or ARX_ERR_NOT_READY changes nothing: a table installed before stays installed
 * (a device error while the new table is uploaded drops it).
 * arx_band_count reports the bands of the installed table (0: none), which is what arx_render_bands will
 * write: size its output buffers from it.  The table is not part of any cache key: the records depend only
 * on the scene's own absorption.
 *
 * arx_render_bands' outputs follow arx_render_listeners': ir_left / ir_right n_bands x ir_len floats each,
 * host or device memory copied with hipMemcpyDefault on the renderer's stream (both NULL: no IRs; exactly
 * one NULL is an error), acoustics n_bands x 3 (channel 0, 1, 2 per band; host memory; NULL: no analysis),
 * results one per band (host memory; NULL: none), *ms the device time of the whole call, its warm launches
 * included (a pair of events, recorded only when ms is given).  The call synchronises once, at its end.  Like
 * arx_get_stats it then reads the tree's off-grid flag: if the receiver refit of a listener move put a box
 * outside the quantization grid, the call returns ARX_ERR_INTERNAL instead of finished results.
 *
 * Where the frame comes from.  While the cache holds no recording of the current key, the call first runs
 * ordinary arx_render launches of the current settings -- normally two, never more than three -- and
 * reports their count in warm_launches.  There is NO traced fallback: if the cache cannot hold the launch
 * (cache off; not cacheable: global stack, CW4, f32 nodes; records over arx_debug_set_path_cache's
 * max_bytes, or no room for them on the device) the call returns ARX_ERR_NOT_READY and the message says
 * which -- raise max_bytes to at least arx_debug_path_cache_bytes().  ARX_ERR_NOT_READY also without a
 * scene or without a table.  ARX_ERR_INVALID_ARGUMENT: NULL r, more than one frame in flight, a caller's
 * own stream (arx_set_stream), an attached histogram.  Only the 24-B records and the cache's direction copy
 * are read: the path filter may be on or off.
 *
 * What the call leaves alone: the renderer's last frame (arx_copy_ir, arx_get_stats, arx_get_acoustics, the
 * IR generation streams follow) is untouched when no warm launch ran, else it is the last warm launch's;
 * the listener, the records and the path filter's state stay.
 *
 * Memory, OUTSIDE arx_debug_set_path_cache's max_bytes (arx_debug_band_bytes): the device table,
 * n_tris x W x 4 B with W = 4 for up to four bands and 8 beyond (a hit fetches its bands in one or two 16-B
 * loads), and one scratch allocation per renderer -- per band 16 x ir_len (histogram) + 64 (counter block)
 * + 336 (three arx_acoustics) + 8 x ir_len (f32 IR pair) B, then one decay-curve buffer of 24 x ir_len B
 * and the analysis kernels' scratch (arx_debug_band_bytes(0, 0, 1) - 400).  Both are kept across calls and
 * freed when they must grow and at arx_destroy.
 *
 * This call's replay is unfiltered and serves the renderer's one listener; the filtered band replay, for a
 * batch of listeners, is arx_render_listener_bands (below).  Out of scope: groups, the C++ shim and app.py
 * modes. */
#define ARX_MAX_BANDS 8
/* table[b * n_tris + t]: band b's absorption of scene triangle t (arx_set_scene's order). n_bands 0 drops it. */
arx_status arx_set_band_absorption(arx_renderer* r, const float* table, int32_t n_bands, int64_t n_tris);
/* bands of the installed table: 0 without one (and for a NULL r) */
int32_t arx_band_count(const arx_renderer* r);
/* host only: the rule above, checked; *bad_band / *bad_tri name the first offender (-1 / -1: none; either may be NULL) */
arx_status arx_band_table_check(const float* scene_absorption, const float* table, int32_t n_bands,
                                int64_t n_tris, int32_t* bad_band, int64_t* bad_tri);
typedef struct arx_band_result {                                                         /* 40 B, no implicit padding */
    uint64_t queries, receiver_hits, misses;   /* arx_stats' counters of this band's frame */
    int32_t warm_launches;                     /* ordinary launches the call ran first to get a recording (same in every entry) */
    int32_t reserved;                          /* 0 */
    uint64_t reserved2;                        /* 0 */
} arx_band_result;
arx_status arx_render_bands(arx_renderer* r, float* ir_left, float* ir_right,  /* n_bands*ir_len each, or both NULL */
                            arx_acoustics* acoustics,                          /* n_bands*3, or NULL */
                            arx_band_result* results,                          /* n_bands, or NULL */
                            double* ms);                                       /* device time of the whole call, or NULL */
/* host only: bytes of the table and the scratch above (0 for n_bands outside [1, ARX_MAX_BANDS]) */
uint64_t arx_debug_band_bytes(int32_t ir_len, int64_t n_tris, int32_t n_bands);

/* Band synthesis: one broadband IR pair from the band IRs, on the device.
 *
 * arx_render_bands gives every band's IR; arx_set_ir_device, the file convolution, the streams and
 * arx_convolute_walk take one IR pair.  arx_combine_bands is the step between them: each band's IR filtered
 * with that band's FIR filter, the bands summed, one f32 IR pair written.  An IR here is the energy
 * histogram used directly as convolution taps (the reference's semantics), and the combine is the linear map
 * out = sum_b g_b (*) ir_b on those taps.  With equal bands and a bank that sums to a unit impulse the result
 * is the single-band IR again.
 *
 * The arithmetic, fixed so that results can be compared on bits.  With c = (taps - 1) / 2, for each ear and
 * each n in [0, ir_len):
 *
 *   for b in 0 .. n_bands-1:
 *       acc_b = +0.0
 *       for k in 0 .. taps-1, ascending:
 *           m = n + c - k
 *           if 0 <= m < ir_len: acc_b = fma(g_b[k], (double)ir_b[m], acc_b)      one f64 fma
 *   s = acc_0; for b in 1 .. n_bands-1: s = s + acc_b
 *   out[n] = (float)s                                                            one rounding to f32
 *
 * So the result is zero-phase: the filters' delay c is taken out, and samples outside [0, ir_len) read as
 * zero.  (A zero input leaves acc_b's bits as they are -- acc_b is never -0.0 -- so the kernel feeds zeros
 * for them and skips stretches that lie wholly outside.)  No band's sum is split over several accumulators
 * and no order is changed.  The filters must be finite: that is the caller's duty and is not checked on the
 * device.  Outputs that overlap inputs are undefined.
 *
 * arx_band_filters (host only) designs the one filter bank everyone gets: n_bands linear-phase FIR filters
 * of `taps` coefficients whose sum is a unit impulse at c.  With N the smallest power of two >= 4 taps and
 * the grid f_m = m sample_rate / N, m = 0 .. N/2: the low-pass of crossover x_i is L_i(0) = 1 and otherwise,
 * with u = log2(f / x_i), 1 for u <= -1/2, 0 for u >= 1/2 and (1 - sin(pi u)) / 2 between -- a raised cosine
 * one octave wide in log-frequency; L_-1 = 0, L_(n_bands-1) = 1 and G_b = L_b - L_(b-1), so G_b >= 0 and the
 * G_b sum to 1.  For j = 0 .. c: h_b[j] = (1/N) sum_m w_m G_b(f_m) cos(2 pi r / N) with r = (m j) mod N in
 * integers, w_0 = w_(N/2) = 1 and every other w_m = 2, m ascending; win[j] = (1 + cos(pi j / (c + 1))) / 2
 * (Hann); g_b[c + j] = g_b[c - j] = h_b[j] win[j], one value stored twice.  ARX_ERR_INVALID_ARGUMENT: NULL
 * g; NULL crossovers with n_bands > 1; n_bands outside [1, ARX_MAX_BANDS]; taps even or outside
 * [1, ARX_BAND_TAPS_MAX]; sample_rate <= 0; a crossover that is not finite, not positive, not strictly
 * ascending, or >= sample_rate / 2.
 *
 * arx_combine_bands follows arx_convolute_walk: it needs no scene; ir_left / ir_right (n_bands x ir_len
 * floats each, arx_render_bands' layout; ir_len is the caller's, not the renderer's), filters (n_bands x taps
 * doubles) and out_left / out_right (ir_len floats each) may each be host or device memory on the renderer's
 * device and are copied with hipMemcpyDefault on the renderer's stream; the call orders itself on that
 * stream, synchronises once, at its end, and reports in *ms its device time, copies included (a pair of
 * events; recorded when ms is given or arx_set_timing is on).  It leaves the renderer's IR, its IR
 * generation, its streams, its listener, its path cache and arx_render_bands' scratch alone.
 * ARX_ERR_INVALID_ARGUMENT: NULL r, ir_left, ir_right, filters, out_left or out_right; n_bands outside
 * [1, ARX_MAX_BANDS]; taps even or outside [1, ARX_BAND_TAPS_MAX]; ir_len 0 or above INT32_MAX; a caller's
 * own stream (arx_set_stream), as in arx_render_bands.  ARX_ERR_OUT_OF_MEMORY when the scratch cannot be
 * allocated; the renderer stays usable.
 *
 * Memory, OUTSIDE arx_debug_set_path_cache's max_bytes: one scratch allocation per renderer, made by the
 * first call, kept across calls, freed when it must grow and at arx_destroy.  A call needs
 * (arx_debug_combine_bytes), every term rounded up to a multiple of 256:
 *   2 x (4 n_bands ir_len)   the band IRs, left and right
 *   + 8 n_bands taps         the filters
 *   + 2 x (4 ir_len)         the outputs, left and right
 * (8 bands, 48 kHz x 2 s, 4095 taps: 7.2 MB.)
 *
 * One IR set per call; several sets (listeners x bands) are combined inside arx_render_listener_bands
 * (below).  Not offered: groups, the C++ shim, app.py modes, filters longer than ARX_BAND_TAPS_MAX. */
#define ARX_BAND_TAPS_MAX 8191
/* host only: g[b * taps + k], band b's filter; crossovers_hz n_bands - 1 values, ascending (NULL with one band) */
arx_status arx_band_filters(int32_t sample_rate, const double* crossovers_hz, int32_t n_bands, int32_t taps,
                            double* g);
arx_status arx_combine_bands(arx_renderer* r,
                             const float* ir_left, const float* ir_right, /* n_bands x ir_len each */
                             int32_t n_bands, size_t ir_len,
                             const double* filters, int32_t taps,          /* n_bands x taps */
                             float* out_left, float* out_right,           /* ir_len each */
                             double* ms);                                 /* device time of the call, or NULL */
/* host only: scratch bytes of a call by the formula above; 0 for arguments the call rejects */
uint64_t arx_debug_combine_bytes(size_t ir_len, int32_t n_bands, int32_t taps);

/* Band IRs for a batch of listeners in one call, from one recorded path set.
 *
 * arx_render_listeners answers many listeners for the scene's one absorption; arx_render_bands answers every
 * band for the renderer's one listener.  arx_render_listener_bands joins them: entry (j, b) of its outputs
 * is, bit for bit, what this loop gives,
 *
 *   saved = listener
 *   for j in 0..n-1: arx_set_listener(poses[j]); arx_render_bands(...); [arx_combine_bands(set j, filters)]
 *   arx_set_listener(saved)
 *
 * -- both IR channels, the three counters, the three arx_acoustics and the broadband pair -- and so, by
 * arx_render_bands' contract, the frame of a renderer at pose j whose scene carries table[b].  ir_left /
 * ir_right are [listener][band][ir_len] (n x n_bands x ir_len floats each, n_bands = arx_band_count; host or
 * device memory; both NULL: no band IRs); with `filters` (arx_band_filters' n_bands x taps doubles, host or
 * device memory) bb_left / bb_right take one broadband pair per listener, [listener][ir_len] --
 * arx_convolute_walk's layout -- each arx_combine_bands of that listener's bands; acoustics n x n_bands x 3
 * and results n x n_bands are host memory (NULL: none); *ms the device time of the whole call, its warm
 * launches included (recorded only when ms is given).  n == 0: ARX_OK, nothing is touched.
 *
 * How.  The batched route is arx_render_listeners' -- chunks of receiver slots, one refit, one filter pass
 * over the stored segments for eight listeners at a time, the listeners' work items -- with a band chain as
 * the candidate kernel.  A candidate query's energy per band needs the chain of the ray's earlier hits:
 * those are the recorded triangle ids, one 16-B record load and one table row each, with no geometry (the
 * position, distance and direction before every query are in the filter's planes), so a candidate ray is
 * walked once from bounce 0 and only its candidate bounces run the receiver query.  A band's query count
 * needs every ray: base_b(ray), the queries band b makes along the ray's scene-only recording, does not
 * depend on the listener and is counted once per call for all rays (8 B per ray); a ray that a listener's
 * receiver ends at query k took exactly max(0, base_b(ray) - (k + 1)) queries of band b away, and only
 * candidate rays can be ended, so per listener and band queries = sum over all rays of base_b - sum over
 * the ended rays of max(0, base_b - (k + 1)).  A flagged last query (a miss, or a scene triangle marked as
 * receiver) is always a candidate and always the ray's last recorded query: it cuts nothing.  Per chunk
 * then, per (listener, band), a finalize and, when asked, an analysis; with filters one band synthesis per
 * listener; the copies.  The batched route synchronises once, at the call's end.
 *
 * Routing.  No recording of the current key yet: warm launches as in arx_render_bands, at poses[0],
 * counted in warm_launches.  Cache off, launch not cacheable or records over the cap: ARX_ERR_NOT_READY, as
 * in arx_render_bands; also without a scene or without a table.  A recording without filter state (filter
 * off, no room for its planes, max_bounces > 64), a receiver too large for the device refit, or no room
 * for the scratch: every pose takes the one-listener route -- arx_set_listener + arx_render_bands
 * (+ arx_combine_bands) inside the call, each ending synchronised -- and reports ARX_LISTENER_SINGLE.  A
 * single pose takes it in place when the emitter lies inside its grown receiver box or its receiver cannot
 * be put on the quantization grid.  Before the first chunk the grid is grown once to hold every pose's
 * receiver.  A slot refit that leaves the grid ends the call with ARX_ERR_INTERNAL.
 *
 * ARX_ERR_INVALID_ARGUMENT: arx_render_listeners' cases (NULL r, NULL poses with n > 0, exactly one IR
 * pointer NULL, a non-finite pose, more than one frame in flight, a caller's own stream, an attached
 * histogram); exactly one of bb_left / bb_right NULL; filters without the bb pair or the pair without
 * filters; with filters, taps even or outside [1, ARX_BAND_TAPS_MAX].
 *
 * What the call leaves alone: the renderer's last frame (untouched when no warm launch ran, else the last
 * warm launch's), the records and the path filter's state; the listener is restored.  It may overwrite the
 * scratch of arx_render_bands and of arx_combine_bands (the one-listener route).
 *
 * Memory, OUTSIDE arx_debug_set_path_cache's max_bytes: one scratch allocation per renderer of its own,
 * made by the first batched call, kept across calls, freed when it must grow and at arx_destroy.
 * arx_debug_listener_band_bytes(rays, ir_len, recv_nodes, recv_tris, n_bands, listeners) is
 *   listeners x ( 96 x recv_nodes + 48 x recv_tris + 96 + 112    the receiver slot, its top node, the table entry
 *               + 16 x rays + 16 x ceil(rays/1024)               the candidate list and its heads
 *               + 16 + 64 x ceil(rays/1024)                      the candidate launch's work items
 *               + n_bands x (16 x ir_len + 64 + 336 + 8 x ir_len)  per band: histogram, counter block, three
 *                                                                arx_acoustics, f32 IR pair
 *               + 64 + 8 x ir_len )                              the candidate tally's block, the broadband pair
 *   + 8 x rays + 512                                             once per call: the per-ray band counts, the
 *                                                                base counter block
 * plus, not counted, one decay-curve buffer of 24 x ir_len B, the analysis kernels' scratch and the filter
 * bank.  arx_debug_set_listener_chunk applies; the automatic chunk is the largest count, at most 64, that
 * keeps the formula within the same 512 MiB: at 1M rays, a 2-s IR at 48 kHz, the 1 020-triangle head and 8
 * bands, 35.4 MB per listener, so 14 listeners (481 MiB; 15 would be 514.4 MiB).  0 for negative arguments or n_bands outside
 * [1, ARX_MAX_BANDS].
 *
 * Not offered here: groups, the C++ shim, app.py modes and frames in flight. */
typedef struct arx_listener_band_result {                                                /* 48 B, no implicit padding */
    uint64_t queries, receiver_hits, misses;   /* arx_stats' counters of this (listener, band)'s frame */
    uint64_t candidate_rays;                   /* batched route only (the same in every band of a listener), else 0 */
    int32_t route;                             /* ARX_LISTENER_BATCHED / ARX_LISTENER_SINGLE */
    int32_t warm_launches;                     /* as arx_band_result's, the same in every entry */
    uint64_t reserved2;                        /* 0 */
} arx_listener_band_result;
arx_status arx_render_listener_bands(arx_renderer* r, const arx_listener_pose* poses, size_t n,
                                     float* ir_left, float* ir_right,     /* [listener][band][ir_len], or both NULL */
                                     const double* filters, int32_t taps, /* n_bands x taps, or NULL / 0 */
                                     float* bb_left, float* bb_right,     /* [listener][ir_len]; required iff filters */
                                     arx_acoustics* acoustics,            /* n*n_bands*3, or NULL */
                                     arx_listener_band_result* results,   /* n*n_bands, or NULL */
                                     double* ms);                         /* device time of the whole call, or NULL */
/* host only: the formula above */
uint64_t arx_debug_listener_band_bytes(uint64_t n_rays, int32_t ir_len, int64_t recv_nodes, int64_t recv_tris,
                                       int32_t n_bands, int32_t listeners);

/* Directional sources: a directivity pattern per band on the band replays.
 *
 * A voice, a loudspeaker or an instrument radiates unevenly, more so the higher the band, and can be turned.
 * A ray's geometry does not depend on its energy, the path cache's records hold the scene-only closest hit
 * of every query of every ray, and the cache keeps a copy of the rays' initial directions.  So a pattern
 * changes one thing: the energy a ray's band b starts with, e[b] = e0 * g[ray][b] instead of e0, in the
 * kernels that already carry one energy per band.  Gains lie in [0, 1] and the f32 product by one is
 * monotone, so a band's energy still never exceeds the recorded ray's at the same bounce (the argument above
 * arx_set_band_absorption, now from e0 * g <= e0): every query a directed band runs has a record.  Neither
 * the pattern nor the orientation is part of any cache key: installing, swapping or turning a pattern costs
 * one small kernel (the gain plane) and a replay, never a trace and never a scene build.
 *
 * The pattern is a cube map per band, cube[((b * 6 + face) * res + v) * res + u], f32 in [0, 1], n_bands 1
 * (serves every band of the table) or up to ARX_MAX_BANDS, res in [1, 256].  A NaN or a value outside [0, 1]
 * is ARX_ERR_INVALID_ARGUMENT and arx_last_error() names the band and the texel.  A cube map and not a
 * latitude / longitude grid because its lookup needs no acos / atan2.
 *
 * The lookup is defined on bits: IEEE f32 add, mul, div and comparisons only, in the order written, never
 * contracted.  arx_directivity_gains_host is that definition in plain C++ and the device runs the same
 * function.  For a ray's initial direction d and the orientation m (9 floats; row i is the source's local
 * axis i -- x, y, z -- in world coordinates; identity by default; arx_set_source_orientation checks in f64
 * that the rows are orthonormal to 1e-5):
 *   l_i = (m[3i] * d.x + m[3i+1] * d.y) + m[3i+2] * d.z;   ax, ay, az = |l.x|, |l.y|, |l.z|
 *   ax >= ay && ax >= az:  face = l.x >= 0 ? 0 : 1,  (sc, tc, ma) = (l.y, l.z, ax)
 *   else ay >= az:         face = l.y >= 0 ? 2 : 3,  (sc, tc, ma) = (l.x, l.z, ay)
 *   else:                  face = l.z >= 0 ? 4 : 5,  (sc, tc, ma) = (l.x, l.y, az)
 *   u = sc / ma, v = tc / ma;  iu = min(res - 1, (int)((u + 1.0f) * (0.5f * (float)res))), iv likewise from v
 *   g[b] = cube[b][face][iv][iu];  ma == 0 (the zero vector; also a NaN): g = 0.
 * This is the project's own convention: faces +x, -x, +y, -y, +z, -z, and NO per-face sign flips -- on every
 * face u and v grow with the two remaining local coordinates in x, y, z order.  Nearest texel, no
 * interpolation.  The engine does not renormalise: gains <= 1 radiate less than the omnidirectional source,
 * and a caller who wants equal radiated power scales base_power by the pattern's mean gain.
 *
 * Who honours it: arx_render_bands and arx_render_listener_bands (one band whose table is the scene's own
 * absorption is the broadband directed render).  arx_render, arx_render_listeners, the warm launches of the
 * band calls and renderer groups stay omnidirectional.  With no pattern installed the band calls launch the
 * same kernel instantiations as before.  At render time a pattern of more than one band must have as many
 * bands as the table (arx_band_count), else ARX_ERR_INVALID_ARGUMENT.  The pattern and the orientation survive
 * arx_set_scene and arx_set_band_absorption; n_bands 0 drops the pattern.  A call that fails with
 * ARX_ERR_INVALID_ARGUMENT or ARX_ERR_NOT_READY changes nothing (a device error while a new pattern is
 * uploaded drops it).  A band whose start fails e[b] > energy_thres never lives: it counts no query, hit or
 * miss -- with gain 0 even at energy_thres 0.
 *
 * The gain plane g[slot][W] (W = 4 for up to four bands, 8 beyond; the padding 0; slot indexes the cache's
 * direction copy) is made by the first band call that needs it and remade only when the pattern, the
 * orientation, the band count or the recording has changed since.  Memory, OUTSIDE arx_debug_set_path_cache's
 * max_bytes (arx_debug_directivity_bytes): the plane, n_rays x W x 4 B, and the cube, n_bands x 6 x res x res
 * x 4 B; kept across calls, freed when they must grow and at arx_destroy.  Out of scope: groups, the C++ shim,
 * app.py modes, interpolated lookup, receiver directivity. */
arx_status arx_set_source_directivity(arx_renderer* r, const float* cube, int32_t n_bands, int32_t res);
arx_status arx_set_source_orientation(arx_renderer* r, const float* m9);
/* bands of the installed pattern: 0 without one (and for a NULL r) */
int32_t arx_source_directivity_bands(const arx_renderer* r);
/* host only, the lookup's definition: out[i * width + b] for n directions (x, y, z each); width 4 or 8 and at
 * least n_bands; a one-band cube fills all `width` columns, else the columns past n_bands are 0; m9 NULL:
 * identity.  The cube and m9 are checked as the setters check them. */
arx_status arx_directivity_gains_host(const float* cube, int32_t n_bands, int32_t res, const float* m9,
                                      const float* dirs_xyz, uint64_t n, int32_t width, float* out);
/* rows [first_ray, first_ray + count) of the device plane (W floats each, W from the band count the next band
 * call runs with: the table's, or the pattern's without a table), made now from the current recording if it is
 * stale.  ARX_ERR_NOT_READY without a pattern or without a recording. */
arx_status arx_debug_directivity_plane(arx_renderer* r, uint64_t first_ray, uint64_t count, float* h_out);
/* host only: the formula above (0 for arguments out of range) */
uint64_t arx_debug_directivity_bytes(uint64_t n_rays, int32_t n_bands, int32_t res);
/* gain planes made so far (launches of the gain kernel) */
uint64_t arx_debug_directivity_planes_made(const arx_renderer* r);
/* the raw fixed-point histograms of the last finished arx_render_bands call, band b's [L | R] at
 * h_out + b * 2 * ir_len, before finalize; capacity in words.  ARX_ERR_NOT_READY before the first call. */
arx_status arx_debug_band_histograms(arx_renderer* r, int64_t* h_out, size_t capacity);

/* Air absorption: an attenuation per band and path length on the band replays.
 *
 * Air attenuates sound with distance, and strongly with frequency: at 20 C and 50 % relative humidity about
 * 4.7 dB/km at 1 kHz, 30 dB/km at 4 kHz and 105 dB/km at 8 kHz (ISO 9613-1's formula,
 * arx_air_absorption_iso9613).  A ray's geometry does not depend on its energy, so the path cache's records
 * serve unchanged: the attenuation is one factor per (band, receiver hit), applied where a band's energy is
 * deposited.  The coefficients are part of no cache key: installing, changing or dropping them costs one small
 * host loop, one upload and a replay, never a trace, a recording or a scene build.
 *
 * Coefficients: alpha[b], the loss in dB per metre, f64, finite and >= 0; n is 1 (one value serves every band
 * of the table) or up to ARX_MAX_BANDS.  A NaN, a negative or an infinite value is ARX_ERR_INVALID_ARGUMENT and
 * arx_last_error() names the band.  A band takes whatever the caller gives it -- its centre frequency's
 * pure-tone value from arx_air_absorption_iso9613, or a band-integrated coefficient of the caller's own.
 *
 * The attenuation is a table per IR bin and band, made on the host in f64 from the renderer's sample_rate and
 * ir_len (both fixed at arx_create):
 *   d_k       = ((double)k * 343.0) / (double)sample_rate                  k = 0 .. ir_len-1
 *   att[k][b] = (float)exp(-((alpha[b] * 0.23025850929940458) * d_k))
 * d_k is the path length that lands in bin k under the engine's rule k = roundf(dist / 343 * sample_rate), so
 * the table is off from a hit's true distance by at most half a sample of path (at 0.1 dB/m and 16 kHz about
 * 0.001 dB).  The speed of sound stays 343 m/s.  alpha >= 0 gives att <= 1: a deposit never grows, and the
 * int64 histogram's headroom holds as it stands.  att[0][b] is exactly 1.0f, and with alpha[b] == 0 every
 * entry of band b is exactly 1.0f.  libm's exp is not correctly rounded, so it is the TABLE that is defined on
 * bits: arx_air_attenuation_host returns it, and the device holds the same bytes (arx_debug_air_table).
 *
 * Where it enters: only at a hit on a receiver half with bin k < ir_len, for a live band b --
 *   ea = e[b] * att[k][b]                                        one f32 product
 *   own ear:    bin k,  ea
 *   other ear:  bin kk, ea * (1.0f - hrtf)                        (stereo only; kk = k + delay, folded to k)
 * Both ears take att at k, not at kk: the interaural delay is the head's, not the path's.  A dropped hit
 * (k >= ir_len) reads no row.
 * What stays the same -- the convention: the energy a band carries along its ray is unchanged (e[b], the
 * e[b] > energy_thres guard, which queries a band runs).  Air absorption weights arrivals and NEVER ends a
 * ray, so per band the three counters (queries, receiver_hits, misses) are exactly those of the call without
 * air, and every query a band runs still has a record.
 *
 * Who honours it: arx_render_bands and arx_render_listener_bands (its one-listener route and its broadband
 * pairs included) and what is built on them.  arx_render, arx_render_listeners, the warm launches of the band
 * calls and renderer groups stay without air.  With no coefficients installed the band calls launch the same
 * kernel instantiations as before.  At render time more than one coefficient must be as many as the table's
 * bands (arx_band_count), else ARX_ERR_INVALID_ARGUMENT.  The coefficients survive arx_set_scene and
 * arx_set_band_absorption; n 0 drops them.  A call that fails with ARX_ERR_INVALID_ARGUMENT or
 * ARX_ERR_NOT_READY changes nothing.  Coefficients and a source pattern may be installed together: the pattern
 * sets the energy a band starts from, the air factor applies at the deposit.
 *
 * The device table att[bin][W] (W = 4 for up to four bands, 8 beyond; the padding 0, or every column filled
 * for one coefficient) is made by the first band call that needs it and remade only when the coefficients or
 * the call's band count have changed since.  Memory, OUTSIDE arx_debug_set_path_cache's max_bytes
 * (arx_debug_air_bytes): ir_len x W x 4 B, 3 MB at 96 000 bins and W = 8; kept across calls, freed when it must
 * grow and at arx_destroy.  Out of scope: groups, the C++ shim, app.py modes, air absorption on arx_render and
 * arx_render_listeners, a temperature-dependent speed of sound (the distance limit, and so the recording,
 * depends on it), per-hit instead of per-bin attenuation, air absorption as a reason to end a ray. */
arx_status arx_set_air_absorption(arx_renderer* r, const double* alpha_db_per_m, int32_t n); /* n 0 drops */
/* coefficients installed: 0 without any (and for a NULL r) */
int32_t arx_air_absorption_bands(const arx_renderer* r);
/* host only, the table's definition: out[k * width + b]; width 4 or 8 and at least n; n == 1 fills all `width`
 * columns, else the columns at and past n are 0; sample_rate and ir_len positive.  The coefficients are checked
 * as the setter checks them. */
arx_status arx_air_attenuation_host(const double* alpha_db_per_m, int32_t n, int32_t sample_rate, int32_t ir_len,
                                    int32_t width, float* out);
/* host only: ISO 9613-1's pure-tone attenuation in dB/m at each of n frequencies.  With T = temperature_c +
 * 273.15, T0 = 293.15, T01 = 273.16, p = pressure_kpa / 101.325, f in Hz:
 *   C   = -6.8346 (T01/T)^1.261 + 4.6151;   h = relative_humidity_percent 10^C / p
 *   frO = p (24 + 4.04e4 h (0.02 + h) / (0.391 + h))
 *   frN = p (T/T0)^(-1/2) (9 + 280 h exp(-4.170 ((T/T0)^(-1/3) - 1)))
 *   alpha = 8.686 f^2 (1.84e-11 / p (T/T0)^(1/2) + (T/T0)^(-5/2) (0.01275 exp(-2239.1/T) / (frO + f^2/frO)
 *                                                                + 0.1068 exp(-3352.0/T) / (frN + f^2/frN)))
 * Accepted: temperature in [-20, 50] C, humidity in [0, 100] %, pressure in (0, 200] kPa, f > 0; anything else,
 * or non-finite, is ARX_ERR_INVALID_ARGUMENT. */
arx_status arx_air_absorption_iso9613(double temperature_c, double relative_humidity_percent, double pressure_kpa,
                                      const double* freq_hz, int32_t n, double* alpha_db_per_m);
/* rows [first_bin, first_bin + count) of the device table (W floats each, W from the band count the next band
 * call runs with: the table's, or the coefficients' without a band table), made now if it is stale.  The table
 * depends on no recording, so none is needed; ARX_ERR_NOT_READY without coefficients. */
arx_status arx_debug_air_table(arx_renderer* r, int64_t first_bin, int64_t count, float* h_out);
/* host only: the formula above (0 for n_bands outside 1..ARX_MAX_BANDS or a negative ir_len) */
uint64_t arx_debug_air_bytes(int32_t ir_len, int32_t n_bands);
/* attenuation tables made so far (uploads) */
uint64_t arx_debug_air_tables_made(const arx_renderer* r);

/* Walk-through convolution: one signal against a per-block IR schedule, in one call.
 *
 * ir_left / ir_right hold n_irs IRs of ir_len frames each (arx_render_listeners' layout; ir_len and the
 * sample rate are the renderer's), ir_of_block[b] in [0, n_irs) names the IR of output block b (host
 * memory), in holds n_frames <= n_blocks * block_frames f64 frames, out receives 2 * n_blocks *
 * block_frames doubles, zipped L/R.  ir_left, ir_right, in and out may each be host or device memory on
 * the renderer's device: they are copied with hipMemcpyDefault on the renderer's stream, as
 * arx_render_listeners copies its IRs.  The call needs no scene.  With B = block_frames, F = fade_frames,
 * the output is bit for bit that of this loop, run on a fresh stream of the same renderer:
 *
 *   s = arx_stream_create(r, B); arx_stream_set_crossfade(s, F, fade_shape)
 *   for b in 0 .. n_blocks-1:
 *       j = ir_of_block[b]
 *       if b == 0 or j != ir_of_block[b-1]: arx_set_ir_device(r, ir_left + j*ir_len, ir_right + j*ir_len, ir_len)
 *       m = clamp(n_frames - b*B, 0, B)
 *       arx_stream_process_device(s, m ? in + b*B : NULL, m, out + 2*b*B)
 *
 * So block b > 0 is a transition block exactly when F > 0 and ir_of_block[b] != ir_of_block[b-1]: it
 * fades from the previous block's IR to its own over its first F frames with arx_stream_fade_weights'
 * values; with F == 0 an IR change is the hard switch; blocks past the input ring out the tail
 * (arx_walk_blocks counts them).  Unlike the loop the call leaves the renderer alone: its IR, its IR
 * generation, its arx_stream objects, its listener and its path cache do not change, and a live stream of
 * the same renderer produces the same bits with or without a walk call in between.  The call orders
 * itself on the renderer's stream as arx_stream_process_device does, synchronises once, at its end, and
 * reports in *ms its device time, copies included (a pair of events; recorded when ms is given or
 * arx_set_timing is on).
 *
 * How: nothing runs block after block.  The distinct IRs the schedule names are transformed once each
 * (one named several times, A B A included, once; one never named not at all), every block's input
 * spectrum is made in one launch, one multiply-accumulate launch covers every (block, IR) item -- a
 * transition block is two items -- in tiles of consecutive items that share the input spectra they read,
 * one launch inverts every item and one blends every transition block.  Per item the arithmetic is the
 * stream's kernels' (DESIGN.md section 6.6).
 *
 * n_blocks == 0: ARX_OK, nothing is touched.  ARX_ERR_INVALID_ARGUMENT: NULL r, ir_left, ir_right,
 * ir_of_block or out; NULL in with n_frames > 0; n_irs == 0; an index outside [0, n_irs); n_frames >
 * n_blocks * B; B outside [1, min(4096, ir_len)]; F outside [0, B]; an unknown fade_shape.
 * ARX_ERR_OUT_OF_MEMORY when the scratch cannot be allocated; the renderer stays usable.
 *
 * Memory, OUTSIDE arx_debug_set_path_cache's max_bytes: one scratch allocation per renderer, made by the
 * first call, kept across calls, freed when it must grow and at arx_destroy.  With N = the power of two
 * >= 2 B (at least 16), P = ceil(ir_len / B), U = the distinct IRs named, T = the transition blocks,
 * a call needs (arx_debug_walk_bytes), every term rounded up to a multiple of 256:
 *   16 N                    the twiddles
 *   + 8 F                   the fade weights
 *   + 16 N x P x U          the IRs' partition spectra
 *   + 16 N x n_blocks       the input spectra
 *   + 16 N x (n_blocks + T) the accumulated spectrum of every item
 *   + 16 F x T              the previous IR's faded frames
 *   + 8 ir_len x U          the named IRs, f32 left and right
 *   + 8 B x n_blocks        the input frames
 *   + 16 B x n_blocks       the output frames
 *   + 16 (n_blocks + T)     the item tables
 * (48 kHz x 2 s, B = 4096, 728 blocks over 64 IRs with a whole-block fade: 525 MB.)
 *
 * Not offered: groups, the C++ shim, app.py modes, fades longer than a block, float32 output. */
arx_status arx_convolute_walk(arx_renderer* r,
                              const float* ir_left, const float* ir_right, size_t n_irs, /* n_irs x ir_len each */
                              const int32_t* ir_of_block, size_t n_blocks,               /* host; values in [0, n_irs) */
                              const double* in, size_t n_frames,                         /* n_frames <= n_blocks * block_frames */
                              int32_t block_frames, int32_t fade_frames, int32_t fade_shape,
                              double* out,                                               /* 2 * n_blocks * block_frames, zipped L/R */
                              double* ms);                                               /* device time of the call, or NULL */
/* Host only: ceil(n_frames / B) + ceil((ir_len - 1) / B), the blocks until the tail of n_frames input
 * frames has rung out; 0 for a non-positive block_frames or ir_len. */
uint64_t arx_walk_blocks(uint64_t n_frames, int32_t block_frames, int32_t ir_len);
/* Host only: n_irs IRs spread evenly over the input.  Block b < n_input_blocks gets
 * min(n_irs - 1, b * n_irs / n_input_blocks) (integer division); later blocks -- the tail -- keep the last
 * input block's value (0 without input blocks).  ARX_ERR_INVALID_ARGUMENT: n_irs == 0 or above INT32_MAX,
 * NULL ir_of_block with n_blocks > 0. */
arx_status arx_walk_even_schedule(uint64_t n_input_blocks, uint64_t n_blocks, size_t n_irs, int32_t* ir_of_block);
/* Host only: scratch bytes of a call by the formula above; 0 for arguments the call would reject. */
uint64_t arx_debug_walk_bytes(int32_t ir_len, int32_t block_frames, uint64_t irs_used, uint64_t n_blocks,
                              uint64_t n_transitions, int32_t fade_frames);
/* items per multiply-accumulate workgroup: 0 = the product's tile (8), else forced, 1..64 */
arx_status arx_debug_set_walk_tile(arx_renderer* r, int32_t blocks);
/* the last call's blocks, transition blocks, distinct IRs transformed, tiles launched and scratch bytes */
arx_status arx_debug_walk_state(arx_renderer* r, uint64_t out5[5]);

/* Debug / parity hooks. */
arx_status arx_debug_ray_directions(uint64_t seed, uint64_t first_ray, uint64_t count, float* h_out_xyz,
                                    int device);
/* Host only: build the scene tree, turn it into the byte image a rank-0 build broadcasts to the
 * other ranks (arx_group_set_scene), read it back and check it is the same tree; returns the tree's
 * content hash (arx_stats::tree_hash) and the image size. */
arx_status arx_debug_scene_roundtrip(const float* tri_vertices, const float* tri_absorption, int64_t n_tris,
                                     uint64_t* tree_hash, uint64_t* image_bytes);
/* The device node arrays as the last trace used them (synchronises): n_nodes coded f32 nodes
 * (64 B each) into cnodes and their 16-bit quantized copy (32 B each, made on the device) into
 * qnodes (either may be NULL), the quantization grid (origin xyz, scale xyz) into grid[6], and the
 * device re-quantizations issued so far into *requants. */
arx_status arx_debug_node_images(arx_renderer* r, void* cnodes, void* qnodes, size_t n_nodes, float* grid,
                                 uint64_t* requants);
/* Tests only: the most triangles the SAH builder may leave in one leaf (process-wide, for the
 * builds that follow; production 2, range 1..15), so leaves of more than two triangles -- which
 * production trees hold only below the builder's depth cap -- can be traced and checked. */
arx_status arx_debug_set_leaf_max(int32_t leaf_max);
/* Host only: build the scene, its 16-bit quantized BVH2 and its 4-wide compressed copy (CW4), and
 * trace n_rays random rays from the emitter through `bounces` specular reflections on the CPU with
 * both traversals (nearest first, f64 slab and triangle tests); out[16]: [0] queries, [1] / [2]
 * BVH2 node steps / triangle tests per query, [3] / [4] the same for CW4, [5] CW4 max stack depth,
 * [6] queries whose two closest hits differ, [7] CW4 nodes, [8] CW4 depth, [9] BVH2 nodes, [10]
 * BVH2 depth, [11] quantization failures, [12] misses, [13] CW4 99.9th-percentile stack depth,
 * [14] CW4 buffer units. */
arx_status arx_debug_wide_stats(const float* tri_vertices, const float* tri_absorption, int64_t n_tris,
                                const float* emitter, int64_t n_rays, int32_t bounces, uint64_t seed, double* out,
                                size_t n_out);
/* Profiling builds only (ARX_TRACE_PROF=1, tools/trace_profile.py): the last trace launch's
 * per-wave records, 16 uint64 per wave (start / end shader clock, rays, queries, node-step slots
 * and lane-steps, leaf phases and lanes, shade phases and lanes, loop iterations, the time the
 * wave's ray range ran out, wave id); ARX_ERR_NOT_READY in the product build. */
arx_status arx_debug_trace_profile(arx_renderer* r, uint64_t* out, size_t n_words, size_t* n_out);
/* Raw device counters of the last trace (n <= 8): [0] queries [1] receiver hits [2] misses. */
arx_status arx_debug_trace_counters(arx_renderer* r, uint64_t* out, size_t n);
/* Host only: the tree-size guard every scene passes (arx_set_scene, arx_group_set_scene): the trace
 * kernel addresses nodes (64 B) and triangle records (48 B) with 31-bit buffer offsets, so n_nodes * 64
 * and n_tris * 48 must stay <= 2^31 - 1 (ARX_ERR_INVALID_ARGUMENT beyond).  The 28-bit triangle index
 * of a leaf code (~(index * 16 + count)) is wider than that limit needs. */
arx_status arx_debug_check_tree_limits(uint64_t n_nodes, uint64_t n_tris);
/* Tests only: the receiver refit kernel's box padding (0 = automatic, the builder's pad).  A pad far
 * beyond the quantization grid's margin makes the refit raise the tree's off-grid flag (its quantized
 * boxes then fall back to whole-axis, still conservative), which arx_get_stats reports as
 * ARX_ERR_INTERNAL until a later tree write (a listener move, a new scene) is clean again. */
arx_status arx_debug_set_refit_pad(arx_renderer* r, float pad);
/* Force the trace kernel's other paths (parity tests of the paths real scenes rarely take): the
 * default is the 16-bit quantized BVH2 with the LDS stack; bit 0 = the f32 coded BVH2 (taken
 * automatically while the emitter is off the quantization grid), bit 1 = the global-memory
 * traversal stack (taken automatically for trees deeper than the LDS stack), bit 3 = the 4-wide
 * compressed tree (CW4, arx_layout.hpp: half the node loads per query, twice the VALU; slower on
 * MI355X, kept as a measured alternative); 0 = automatic. */
arx_status arx_debug_set_trace_path(arx_renderer* r, int path);

/* ---- Input formats (host only, no device needed) ------------------------------------------ */

/* OBJ scene / receiver model: tinyobj v2.0.0 LoadObj with triangulation (R/prebuild/common/
 * 3rdParty/tiny_obj_loader.h:2095-2600) then one mesh per (shape, material id ascending) with
 * (v,n,t) vertex dedup -- loadOBJ (R/prebuild/obj_raytracer/OptixModel.cpp:75-151).
 * mtl_dir NULL = the OBJ's directory (loadOBJ :79).  first_shape_only + forced_name give
 * HalfSphere + place_receiver_half (HalfSphere.cpp:3-31, OptixModel.cpp:197-220): pass
 * mtl_dir = path up to (excluding) the last '/', forced_name "receiver_left"/"receiver_right".
 * Fails (ARX_ERR_IO) when the OBJ has no materials, like the reference's throw. */
typedef struct arx_model arx_model;
arx_status arx_model_load_obj(const char* path, const char* mtl_dir, int first_shape_only,
                              const char* forced_name, arx_model** out);
void arx_model_free(arx_model* m);
int64_t arx_model_mesh_count(const arx_model* m);
int64_t arx_model_material_count(const arx_model* m);
/* tinyobj's shapes.size(), materials.size(), attrib.vertices.size()/3 */
void arx_model_info(const arx_model* m, int64_t* n_shapes, int64_t* n_materials, int64_t* n_positions);
/* Mesh i: TriangleMesh {material_name, vertex, index} (OptixModel.h); pointers live until free. */
arx_status arx_model_mesh(const arx_model* m, int64_t i, const char** name, const float** vertices,
                          int64_t* n_vertices, const int32_t** indices, int64_t* n_triangles);
int64_t arx_model_triangle_count(const arx_model* m);
/* Triangle soup for arx_set_scene (9 floats per triangle, meshes in model order) with
 * getMaterialAbsorption per mesh name (AudioRenderer.cpp:34-56, :455); tri_absorption may be NULL. */
arx_status arx_model_flatten(const arx_model* m, const char* const* names, const float* absorption,
                             size_t n_materials, float* tri_vertices, float* tri_absorption);

/* WAV: AudioFile<float>::load / decodeWaveFile (R/prebuild/obj_raytracer/AudioFile.h:502-640,
 * sample conversion :1242-1269): PCM 8/16/24/32-bit and IEEE float 32.  *samples is malloc'd,
 * channel-major (channels x frames, like AudioFile::samples); release with arx_free. */
arx_status arx_wav_load(const char* path, float** samples, int32_t* channels, int64_t* frames,
                        int32_t* sample_rate, int32_t* bit_depth);
void arx_free(void* p);

/* ---- Output formats (host only) ------------------------------------------------------------ */

/* AudioFile<float>::save as export_audio uses it (main.cpp:709-716; AudioFile.h:842-955):
 * samples channel-major; 32-bit is written as IEEE float, 8/16-bit are clamped to [-1, 1]. */
arx_status arx_wav_save(const char* path, const float* samples, int32_t channels, int64_t frames,
                        int32_t sample_rate, int32_t bit_depth);
/* normalizeToRangeMinusOneToOne (main.cpp:628-651), in place; constant input -> INVALID_ARGUMENT. */
arx_status arx_normalize_min_max(float* data, size_t n);
/* One value per line, std::ostream default float format -- the output_ir_{left,right}.txt and
 * output_convolute_{left,right}.txt dumps (AudioRenderer.cpp:525-567, 720-744). */
arx_status arx_write_float_lines(const char* path, const float* data, size_t n);

/* config.json: Context::loadContext's parameters (R/prebuild/obj_raytracer/Context.cpp:15-164)
 * with its defaults and rounding (unsigned fields and both re_render thresholds and
 * hrtf_absorption_rate are round()ed), parsed with cJSON 1.7.16 semantics (case-insensitive
 * keys, first duplicate wins, trailing text ignored). */
#define ARX_PATH_MAX 1024
#define ARX_NAME_MAX 128
#define ARX_MAX_MATERIALS 256
typedef struct arx_app_config {
    float initial_volume;
    uint32_t ir_length_in_seconds, width, height;
    int32_t write_first_ir_to_file, write_first_output_to_file;
    float re_render_distance_threshold, re_render_angle_threshold;
    int32_t mono;
    char scene_file_path[ARX_PATH_MAX];
    char audio_file_path[ARX_PATH_MAX];     /* "" = live mic input, sample rate 44100 */
    char materials_file_path[ARX_PATH_MAX];
    float initial_receiver_pos[3];
    float initial_emitter_pos[3];
    float base_power;
    float rays[3];                          /* gdt::vec3f; launch dims are int(rays) (LaunchParams.h:24) */
    float ray_energy_threshold;
    uint32_t ray_max_bounces;
    float hrtf_absorption_rate;
    int32_t n_materials;
    char material_names[ARX_MAX_MATERIALS][ARX_NAME_MAX];
    float material_absorption[ARX_MAX_MATERIALS];
} arx_app_config;
void arx_default_app_config(arx_app_config* c);
arx_status arx_parse_app_config(const char* text, size_t len, arx_app_config* c);
arx_status arx_load_app_config(const char* path, arx_app_config* c);

#ifdef __cplusplus
}
#endif
#endif /* ARX_H */
