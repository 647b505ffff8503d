// api.hip -- the extern "C" surface of libbags_raster.so (include/bags_raster.h) and the state-buffer layout.
#include "bags_common.h"
#include <stdio.h>
#include <string.h>
#include <stdarg.h>

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do { hipError_t e_ = (expr);                                                                        \
         if (e_ != hipSuccess) return fail(BAGS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// after a launcher when settings.debug is on: drain the stream so a faulting kernel is attributed correctly
#define DEBUG_SYNC(s, st, what)                                                                         \
    do { if ((s)->debug) { hipError_t e_ = hipStreamSynchronize(st);                                    \
         if (e_ != hipSuccess) return fail(BAGS_ERR_HIP, "debug: %s failed at iteration %d: %s", what, (s)->debug_iter, hipGetErrorString(e_)); } \
    } while (0)

// settings.debug also scans what a call produced for NaN / Inf (the reference's debug flag dumps a snapshot
// when the CUDA op throws; here the op names the first tensor that went non-finite and the iteration it happened in).
__global__ void __launch_bounds__(256) count_nonfinite_kernel(const float* __restrict__ x, size_t n, u32* __restrict__ counter)
{
    u32 bad = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const u32 b = __float_as_uint(x[i]);
        bad += ((b & 0x7F800000u) == 0x7F800000u) ? 1u : 0u;          // exponent all ones: Inf or NaN
    }
    for (int d = 32; d >= 1; d >>= 1) bad += (u32)__shfl_xor((int)bad, d);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(counter, bad);
}
struct ScanItem { const char* name; const float* ptr; size_t n; };
// counters: device words nobody else uses (GeomView::num_rendered[8 ...], 64 words are carved for it); one per item
static int debug_scan(const BagsSettings* s, hipStream_t st, u32* counters, const ScanItem* items, int n_items, const char* phase,
                      int (*failfn)(int, const char*, ...))
{
    if (!s->debug) return BAGS_OK;
    if (n_items > 32) n_items = 32;
    if (hipMemsetAsync(counters, 0, sizeof(u32) * 32, st) != hipSuccess) return failfn(BAGS_ERR_HIP, "debug scan: memset failed");
    for (int i = 0; i < n_items; ++i) {
        if (!items[i].ptr || items[i].n == 0) continue;
        const int grid = (int)((items[i].n + 256 * 16 - 1) / (256 * 16));
        hipLaunchKernelGGL(count_nonfinite_kernel, dim3(grid < 1 ? 1 : (grid > 4096 ? 4096 : grid)), dim3(256), 0, st, items[i].ptr, items[i].n, counters + i);
    }
    u32 host[32];
    if (hipMemcpyAsync(host, counters, sizeof(u32) * 32, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return failfn(BAGS_ERR_HIP, "debug scan: %s", hipGetErrorString(hipGetLastError()));
    for (int i = 0; i < n_items; ++i)
        if (items[i].ptr && host[i])
            return failfn(BAGS_ERR_DEVICE, "debug: %s produced %u non-finite values in %s at iteration %d", phase, host[i], items[i].name, s->debug_iter);
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- stage profiler
// Opt-in (bags_profile_enable): a start/stop hipEvent pair per stage per call, resolved in bags_profile_read.
#include <atomic>
#include <mutex>
#include <vector>
enum Stage { ST_PRE_FWD, ST_DEPTH_SORT, ST_OFFSETS, ST_EMIT, ST_TILE_SORT, ST_RANGES, ST_BLEND_FWD, ST_BLEND_BWD,
             ST_PRE_BWD, ST_POSE_REDUCE, ST_COUNT };
static const char* kStageNames[ST_COUNT] = {"preprocess_fwd", "depth_sort", "offsets_scan", "emit", "tile_sort",
                                            "tile_ranges", "blend_fwd", "blend_bwd", "preprocess_bwd", "pose_reduce"};
struct ProfInterval { int stage; hipEvent_t a, b; };
// The profiler is the library's only mutable global state (everything a call needs lives in the caller's buffers); calls
// from several threads / streams may profile at once, so the lists are guarded.
static std::mutex g_prof_mutex;
static int g_prof_mode = 0;          // 0 off, 1 dominant kernel only (blend_bwd), 2 every stage
static int g_prof_stride = 1;        // mode 1: every n-th launch of the dominant kernel carries events (bags_profile_stride)
static std::atomic<unsigned long long> g_prof_seq{0};
static std::vector<ProfInterval> g_prof_pending;
static std::vector<hipEvent_t> g_prof_free;
static double g_prof_ms[ST_COUNT];
static long long g_prof_calls[ST_COUNT];

static hipEvent_t prof_event()
{
    {
        std::lock_guard<std::mutex> lk(g_prof_mutex);
        if (!g_prof_free.empty()) { hipEvent_t e = g_prof_free.back(); g_prof_free.pop_back(); return e; }
    }
    hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}
thread_local hipEvent_t g_attach_start = nullptr, g_attach_stop = nullptr;     // (bags_common.h: launch_k)
struct ProfScope {
    hipStream_t st; int stage; hipEvent_t a = nullptr, b = nullptr; bool attached = false;
    // mode 2 (every stage, bench.py's separate untimed pass).  attach: the stage is ONE kernel -- the events ride on its dispatch (no
    // packet of their own: what they report is the kernel's time, as rocprofv3 does); otherwise the stage is bracketed by two recorded
    // events.  Mode 1 (the dominant kernel alone, inside bench.py's timed region) is handled in bags_backward.
    ProfScope(int stage_, hipStream_t st_, bool attach = false) : st(st_), stage(stage_) {
        if (g_prof_mode != 2) return;
        a = prof_event();
        if (attach) { b = prof_event(); attached = true; g_attach_start = a; g_attach_stop = b; }
        else (void)hipEventRecord(a, st);
    }
    ~ProfScope() {
        if (!a) return;
        if (attached) {
            const bool taken = (g_attach_start == nullptr && g_attach_stop == nullptr);
            g_attach_start = nullptr; g_attach_stop = nullptr;
            std::lock_guard<std::mutex> lk(g_prof_mutex);
            if (taken) g_prof_pending.push_back({stage, a, b});
            else { g_prof_free.push_back(a); g_prof_free.push_back(b); }       // the launcher launched nothing
            return;
        }
        b = prof_event(); (void)hipEventRecord(b, st);
        std::lock_guard<std::mutex> lk(g_prof_mutex);
        g_prof_pending.push_back({stage, a, b});
    }
};

// ---------------------------------------------------------------------------------------------- buffer carving
// (bags_common.h: Carver.  Each function below is the ONE statement of its buffer's layout: the bags_*_size functions call it with
// a null base, the entry points with the caller's pointer, which is rounded up to 256 here and nowhere else.)
static size_t carve_geom(void* base, int P, GeomView* v)
{
    Carver c(base);
    GeomView g{};
    const size_t n = (size_t)(P > 0 ? P : 1);
    g.nblocks_sort = radix_blocks_for((long long)n);
    g.nblocks_scan = cdiv((long long)n, SCAN_TILE);
    g.depth_key = c.take<u32>(n); g.g2d = c.take<float4>(4 * n); g.rect = c.take<uint2>(n); g.tiles_touched = c.take<u32>(n);
    g.inst_off = c.take<u32>(n); g.keep = c.take<u64>(n); g.shjac = c.take<float>(10 * n); g.rec_count = c.take<u32>(n);
    g.keys_a = c.take<u32>(n); g.keys_b = c.take<u32>(n); g.vals_a = c.take<u32>(n); g.vals_b = c.take<u32>(n);
    g.rank_offset = c.take<u32>(n); g.scan_partials = c.take<u32>((size_t)g.nblocks_scan + 1);
    g.radix_hist = c.take<u32>((size_t)RADIX_BINS * g.nblocks_sort); g.digit_totals = c.take<u32>(RADIX_BINS); g.num_rendered = c.take<u32>(64);
    g.local_off = c.take<u32>(n); g.block_total = c.take<u32>(256); g.block_base = c.take<u32>(256);
    if (v) *v = g;
    return c.used();
}

static int tile_passes(int T) { return (bit_length((u32)(T > 1 ? T - 1 : 1)) + RADIX_BITS - 1) / RADIX_BITS; }

static size_t carve_binning(void* base, long long I, int W, int H, BinView* v, bool binned)
{
    Carver c(base);
    BinView b{};                                             // (what a path does not carve stays null)
    const size_t n = (size_t)(I > 0 ? I : 1);
    const int T = cdiv(W, BAGS_TILE) * cdiv(H, BAGS_TILE);
    b.nblocks_sort = radix_blocks_for((long long)n);
    b.passes = tile_passes(T);
    if (binned) {                                            // tile-binned path: 20 bytes per instance
        b.words = c.take<u64>(n); b.scratch = c.take<u64>(n); b.point_list = c.take<u32>(n);
        b.reach_mask = reinterpret_cast<unsigned short*>(b.words);       // the unsorted words are dead after the per-tile sorts
    } else {
        b.keys_a = c.take<u32>(n); b.vals_a = c.take<u32>(n); b.keys_b = c.take<u32>(n); b.vals_b = c.take<u32>(n);
        b.ranges = c.take<uint2>((size_t)(T > 0 ? T : 1));
        b.radix_hist = c.take<u32>((size_t)RADIX_BINS * b.nblocks_sort); b.digit_totals = c.take<u32>(RADIX_BINS);
        // emission writes the *_b half; pass 0: b -> a, pass 1: a -> b, ...
        b.point_list = (b.passes & 1) ? b.vals_a : b.vals_b;
        b.tile_sorted = (b.passes & 1) ? b.keys_a : b.keys_b;
        b.reach_mask = reinterpret_cast<unsigned short*>((b.passes & 1) ? b.keys_b : b.keys_a);   // the ping-pong half the last pass read
    }
    if (v) *v = b;
    return c.used();
}

static size_t carve_image(void* base, int W, int H, ImgView* v)
{
    Carver c(base);
    ImgView im{};
    const size_t n = (size_t)W * H > 0 ? (size_t)W * H : 1;
    im.final_T = c.take<float>(n); im.n_contrib = c.take<u32>(n);
    const size_t T = (size_t)cdiv(W > 0 ? W : 1, BAGS_TILE) * cdiv(H > 0 ? H : 1, BAGS_TILE);
    im.tile_desc = c.take<uint4>(T); im.n_active = c.take<u32>(64); im.tile_aux = c.take<uint4>(T);
    if (binned_supported(1, (int)T)) {                        // images the tile-binned path can take (<= 32768 tiles)
        im.cnt_rows = c.take<u32>(256 * ((T + 1) / 2)); im.pre = c.take<u32>(256 * T); im.tile_total = c.take<u32>(T);
        im.ranges = c.take<uint2>(T); im.tile_lstart = c.take<u32>(T); im.group_total = c.take<u32>(512);
    }
    if (v) *v = im;
    return c.used();
}

static size_t carve_backward(void* base, int P, long long I, BwdWorkView* v)
{
    Carver c(base);
    BwdWorkView w;
    const size_t n = (size_t)(I > 0 ? I : 1);
    w.partials = c.take<float>(n * PART_FLOATS);
    w.pose_slab = c.take<float>((size_t)cdiv(P > 0 ? P : 1, 256) * POSE_VALS);
    // Dense-scene mode: one byte per record, + the 64 bytes preprocess_bwd reads from a Gaussian's first mark on (the last Gaussian's
    // read runs past the last mark).  launch_blend_bwd clears the WHOLE region, a multiple of 256: a fill of whole units is ONE launch
    // of the runtime's fill kernel -- with an odd tail it was two, ~5.5 us each -- and the bytes behind the last mark are zero.
    const size_t before = c.used();
    w.live_map = c.take<unsigned char>(n + 64);
    w.live_bytes = c.used() - before;
    if (v) *v = w;
    return c.used();
}

// one row of campos sums per (view, workgroup), view-major (sh_colors.hip); the single-view operator is V = 1
static size_t carve_sh_colors(void* base, int P, int V, float** slab)
{
    Carver c(base);
    float* s = c.take<float>((size_t)(V > 0 ? V : 1) * cdiv(P > 0 ? P : 1, 256) * SH_SLAB);
    if (slab) *slab = s;
    return c.used();
}

// ---------------------------------------------------------------------------------------------- validation
static int check_common(const BagsSettings* s, const BagsInputs* in, const BagsState* stt)
{
    if (!s || !in || !stt) return fail(BAGS_ERR_ARG, "null argument struct");
    if (in->P < 0) return fail(BAGS_ERR_ARG, "P < 0");
    if (s->image_width <= 0 || s->image_height <= 0) return fail(BAGS_ERR_ARG, "empty image %dx%d", s->image_width, s->image_height);
    if (cdiv(s->image_width, BAGS_TILE) > 65535 || cdiv(s->image_height, BAGS_TILE) > 65535)
        return fail(BAGS_ERR_ARG, "image too large for 16-bit tile coordinates");
    if (s->sh_degree < 0 || s->sh_degree > 3) return fail(BAGS_ERR_ARG, "sh_degree %d not in 0..3", s->sh_degree);
    if (!s->bg || !s->viewmatrix || !s->projmatrix || !s->intrinsic || !s->campos)
        return fail(BAGS_ERR_ARG, "bg/viewmatrix/projmatrix/intrinsic/campos must be given");
    if (in->P > 0) {
        if (!in->means3D || !in->opacities) return fail(BAGS_ERR_ARG, "means3D/opacities must be given");
        if ((in->shs != nullptr) == (in->colors_precomp != nullptr))
            return fail(BAGS_ERR_ARG, "Please provide excatly one of either SHs or precomputed colors!");
        const bool sr = in->scales && in->rotations;
        if ((in->scales != nullptr) != (in->rotations != nullptr) || sr == (in->cov3D_precomp != nullptr))
            return fail(BAGS_ERR_ARG, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
        if (in->shs_rest && (!in->shs || s->sh_coeffs < 2))
            return fail(BAGS_ERR_ARG, "shs_rest (features_rest) needs shs (features_dc) and sh_coeffs >= 2 (got %d)", s->sh_coeffs);
        if (in->shs && (s->sh_degree + 1) * (s->sh_degree + 1) > s->sh_coeffs)
            return fail(BAGS_ERR_ARG, "sh_degree %d needs %d coefficients, shs holds %d", s->sh_degree,
                        (s->sh_degree + 1) * (s->sh_degree + 1), s->sh_coeffs);
    }
    if (!stt->geom || stt->geom_bytes < bags_geom_size(in->P)) return fail(BAGS_ERR_SIZE, "geom buffer too small");
    if (!stt->image || stt->image_bytes < bags_image_size(s->image_width, s->image_height))
        return fail(BAGS_ERR_SIZE, "image buffer too small");
    return BAGS_OK;
}


// ---------------------------------------------------------------------------------------------- C ABI
extern "C" {

int bags_abi_version(void) { return BAGS_ABI_VERSION; }
#ifndef BAGS_SRC_HASH
#define BAGS_SRC_HASH "unknown"
#define BAGS_KERNEL_COMMIT "unknown"
#endif
const char* bags_build_info(void) { return "src=" BAGS_SRC_HASH " commit=" BAGS_KERNEL_COMMIT; }
const char* bags_last_error(void) { return g_err; }

size_t bags_geom_size(int32_t P) { return carve_geom(nullptr, P, nullptr) + BASE_SLACK; }
size_t bags_binning_size(int64_t I, int32_t W, int32_t H)
{   // the caller does not know which path a call takes: the larger of the two layouts
    const size_t a = carve_binning(nullptr, I, W, H, nullptr, false), b = carve_binning(nullptr, I, W, H, nullptr, true);
    return (a > b ? a : b) + BASE_SLACK;
}
size_t bags_image_size(int32_t W, int32_t H) { return carve_image(nullptr, W, H, nullptr) + BASE_SLACK; }
size_t bags_backward_workspace_size(int32_t P, int64_t I) { return carve_backward(nullptr, P, I, nullptr) + BASE_SLACK; }

// The views of a call's state buffers and its binning path, decided once per entry point.  capacity: what the binning buffer was
// sized for (the entry point has checked binning_bytes against it), or negative when the call does not touch that buffer.
struct StateViews { GeomView g; BinView b; ImgView im; bool binned; };
static StateViews bind_state(const BagsSettings* s, const BagsInputs* in, const BagsState* stt, int64_t capacity)
{
    StateViews v{};
    const int W = s->image_width, H = s->image_height;
    // tile-binned lists (binning.hip) unless the caller asked for the radix path or the problem is outside their limits
    v.binned = s->binning != BAGS_BINNING_RADIX && binned_supported(in->P, cdiv(W, BAGS_TILE) * cdiv(H, BAGS_TILE));
    carve_geom(stt->geom, in->P, &v.g);
    carve_image(stt->image, W, H, &v.im);
    if (capacity >= 0) carve_binning(stt->binning, capacity, W, H, &v.b, v.binned);
    return v;
}

// K1 + everything the instance count needs; leaves it in g.num_rendered (device)
// host_count (optional): device-visible address of the caller's pinned host word; when the tile-binned path takes it, the
// count is written there by the kernel that computes it and *host_written is set (no copy needed)
static int enqueue_prepare(const BagsSettings* s, const BagsInputs* in, const StateViews& v, const BagsForwardOut* out,
                           hipStream_t st, u32* host_count = nullptr, bool* host_written = nullptr)
{
    const GeomView& g = v.g; const ImgView& im = v.im; const bool binned = v.binned;
    { ProfScope ps(ST_PRE_FWD, st, true);
      HIP_TRY(launch_preprocess_fwd(*s, *in, g, out->radii, out->mean2D, st, binned ? &im : nullptr, cdiv(s->image_width, BAGS_TILE))); }
    DEBUG_SYNC(s, st, "preprocess_fwd");
    if (binned) {
        // (block of Gaussians, tile) count matrix -> column prefixes -> tile ranges, instance count, heavy-first tile list
        const int gx = cdiv(s->image_width, BAGS_TILE), gy = cdiv(s->image_height, BAGS_TILE);
        // host_count given (device-visible pinned word, speculative forward): no ranges_order launch -- the emission launch of
        // the second phase computes the ranges itself and delivers the count there
        { ProfScope ps(ST_OFFSETS, st, host_count != nullptr);          // (one kernel unless the count is wanted now: then ranges_order follows)
          HIP_TRY(launch_binned_prepare(g, im, in->P, gx, gx * gy, st, host_count, host_count == nullptr)); }
        if (host_count && host_written) *host_written = true;
        DEBUG_SYNC(s, st, "tile count / prefix / ranges");
        return BAGS_OK;
    }
    // depth order of the Gaussians: 4 stable 8-bit passes over the float bits (positive floats order like u32)
    { ProfScope ps(ST_DEPTH_SORT, st);
      HIP_TRY(launch_radix_sort(g.depth_key, nullptr, g.keys_a, g.vals_a, g.keys_b, g.vals_b, in->P, 32, true,
                                g.radix_hist, g.digit_totals, g.nblocks_sort, st)); }
    DEBUG_SYNC(s, st, "depth sort");
    const u32* sorted_ids = g.vals_b;                     // 4 passes: src->a->b->a->b
    { ProfScope ps(ST_OFFSETS, st); HIP_TRY(launch_offsets_scan(g, sorted_ids, in->P, st)); }
    DEBUG_SYNC(s, st, "offsets scan");
    return BAGS_OK;
}

static int scan_forward(const BagsSettings* s, const BagsInputs* in, const GeomView& g, const BagsForwardOut* out, hipStream_t st)
{
    if (!s->debug) return BAGS_OK;
    const size_t HW = (size_t)s->image_width * s->image_height;
    const ScanItem items[] = {{"rendered_image", out->color, 3 * HW}, {"depth", out->depth, HW}, {"weights", out->weights, HW},
                              {"mean2D", out->mean2D, 2 * (size_t)in->P}};
    return debug_scan(s, st, g.num_rendered + 8, items, 4, "the forward", fail);
}

// emission, per-tile ordering, blend.  n_dev != nullptr: the instance count is read on the device and checked against
// `I` (the capacity the binning buffer was sized for)
static int enqueue_finish(const BagsSettings* s, const BagsInputs* in, const StateViews& v, const BagsForwardOut* out, int64_t I,
                          const u32* n_dev, hipStream_t st, bool speculative = false)
{
    const GeomView& g = v.g; const BinView& b = v.b; const ImgView& im = v.im;
    const int W = s->image_width, H = s->image_height;
    const int gx = cdiv(W, BAGS_TILE), gy = cdiv(H, BAGS_TILE);
    if (v.binned) {
        if (in->P == 0) HIP_TRY(launch_binned_empty(g, im, gx * gy, st));      // no prepare phase ran: an all-empty tile list
        if (I > 0 && in->P > 0) {
            ProfScope ps(ST_TILE_SORT, st, true);
            HIP_TRY(launch_binned_finish(g, im, in->P, gx, gx * gy, b.words, (u32)I, st, speculative));
        } else if (in->P > 0) {
            HIP_TRY(launch_binned_desc_only(im, gx * gy, st));                   // nothing to emit: only the (all-empty) tile list
        }
        DEBUG_SYNC(s, st, "emit / tile sort");
        { ProfScope ps(ST_BLEND_FWD, st, true); HIP_TRY(launch_blend_fwd(*s, g, b, im, *out, st, n_dev, (u32)I, I > 0 && in->P > 0)); }
        DEBUG_SYNC(s, st, "blend_fwd");
        return scan_forward(s, in, g, out, st);
    }
    if (I > 0) {
        { ProfScope ps(ST_EMIT, st); HIP_TRY(launch_emit(g, g.vals_b, in->P, gx, b.keys_b, b.vals_b, (u32)I, st, n_dev, b.ranges, gx * gy)); }
        DEBUG_SYNC(s, st, "emit");
        { ProfScope ps(ST_TILE_SORT, st);
          HIP_TRY(launch_radix_sort(b.keys_b, b.vals_b, b.keys_a, b.vals_a, b.keys_b, b.vals_b, I, b.passes * RADIX_BITS,
                                    false, b.radix_hist, b.digit_totals, b.nblocks_sort, st, n_dev)); }
        DEBUG_SYNC(s, st, "tile sort");
    }
    { ProfScope ps(ST_RANGES, st);
      HIP_TRY(launch_tile_ranges(b.tile_sorted, I, b.ranges, gx * gy, st, n_dev, I > 0));
      HIP_TRY(launch_tile_order(b.ranges, gx * gy, im.tile_desc, im.n_active, st)); }
    DEBUG_SYNC(s, st, "tile ranges");
    { ProfScope ps(ST_BLEND_FWD, st, true); HIP_TRY(launch_blend_fwd(*s, g, b, im, *out, st)); }
    DEBUG_SYNC(s, st, "blend_fwd");
    return scan_forward(s, in, g, out, st);
}

int bags_forward_prepare(const BagsSettings* s, const BagsInputs* in, const BagsState* stt, const BagsForwardOut* out,
                         int64_t* host_num_rendered, void* stream)
{
    int rc = check_common(s, in, stt);
    if (rc) return rc;
    if (!out || (in->P > 0 && !out->radii) || !host_num_rendered) return fail(BAGS_ERR_ARG, "radii / host_num_rendered must be given");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const StateViews v = bind_state(s, in, stt, -1);
    *host_num_rendered = 0;
    if (in->P == 0) return BAGS_OK;
    rc = enqueue_prepare(s, in, v, out, st);
    if (rc) return rc;
    u32 host_I = 0;
    HIP_TRY(hipMemcpyAsync(&host_I, v.g.num_rendered, sizeof(u32), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *host_num_rendered = (int64_t)host_I;
    return BAGS_OK;
}

int bags_forward_finish(const BagsSettings* s, const BagsInputs* in, const BagsState* stt, const BagsForwardOut* out,
                        int64_t I, void* stream)
{
    int rc = check_common(s, in, stt);
    if (rc) return rc;
    if (!out || !out->color) return fail(BAGS_ERR_ARG, "color output must be given");
    if (I < 0 || I > 0xFFFFFFF0ll) return fail(BAGS_ERR_ARG, "num_rendered out of range");
    const int W = s->image_width, H = s->image_height;
    if (!stt->binning || stt->binning_bytes < bags_binning_size(I, W, H)) return fail(BAGS_ERR_SIZE, "binning buffer too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const StateViews v = bind_state(s, in, stt, I);
    // the count is compared with I on the device as well: a caller-supplied I below the true count renders the overflowing
    // lists empty instead of writing past the binning buffer (same guard as the speculative finish)
    return enqueue_finish(s, in, v, out, I, in->P > 0 ? v.g.num_rendered : nullptr, st);
}

int bags_forward_prepare_async(const BagsSettings* s, const BagsInputs* in, const BagsState* stt, const BagsForwardOut* out,
                               uint32_t* host_num_rendered, void* stream)
{
    int rc = check_common(s, in, stt);
    if (rc) return rc;
    if (!out || (in->P > 0 && !out->radii) || !host_num_rendered) return fail(BAGS_ERR_ARG, "radii / host_num_rendered must be given");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const StateViews v = bind_state(s, in, stt, -1);
    if (in->P == 0) {
        HIP_TRY(hipMemsetAsync(v.g.num_rendered, 0, sizeof(u32), st));
    } else {
        // a pinned (page-locked, device-mapped) host word can be written by the kernel that computes the count
        u32* dev_alias = nullptr;
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, host_num_rendered) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer)
            dev_alias = static_cast<u32*>(attr.devicePointer);
        else (void)hipGetLastError();                         // not a registered pointer: fall back to the copy
        bool written = false;
        rc = enqueue_prepare(s, in, v, out, st, dev_alias, &written);
        if (rc) return rc;
        if (written) return BAGS_OK;
    }
    HIP_TRY(hipMemcpyAsync(host_num_rendered, v.g.num_rendered, sizeof(u32), hipMemcpyDeviceToHost, st));
    return BAGS_OK;
}

int bags_forward_finish_speculative(const BagsSettings* s, const BagsInputs* in, const BagsState* stt,
                                    const BagsForwardOut* out, int64_t capacity, void* stream)
{
    int rc = check_common(s, in, stt);
    if (rc) return rc;
    if (!out || !out->color) return fail(BAGS_ERR_ARG, "color output must be given");
    if (capacity < 1 || capacity > 0xFFFFFFF0ll) return fail(BAGS_ERR_ARG, "capacity out of range");
    const int W = s->image_width, H = s->image_height;
    if (!stt->binning || stt->binning_bytes < bags_binning_size(capacity, W, H)) return fail(BAGS_ERR_SIZE, "binning buffer too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const StateViews v = bind_state(s, in, stt, capacity);
    return enqueue_finish(s, in, v, out, capacity, v.g.num_rendered, st, true);
}

int bags_backward(const BagsSettings* s, const BagsInputs* in, const BagsState* stt, const BagsBackwardArgs* a, void* stream)
{
    return bags_backward_ex(s, in, stt, a, nullptr, stream);
}

int bags_backward_ex(const BagsSettings* s, const BagsInputs* in, const BagsState* stt, const BagsBackwardArgs* a, const BagsExtraGrads* x,
                     void* stream)
{
    int rc = check_common(s, in, stt);
    if (rc) return rc;
    // (ABI 11) the depth / weights cotangents: both null is the plain backward
    const float* grad_depth = x ? x->grad_depth : nullptr;
    const float* grad_weights = x ? x->grad_weights : nullptr;
    const bool extra = grad_depth != nullptr || grad_weights != nullptr;
    if (!a) return fail(BAGS_ERR_ARG, "grad_color must be given");
    if (!a->grad_color && !extra) return fail(BAGS_ERR_ARG, "grad_color must be given (or, with bags_backward_ex, grad_depth / grad_weights)");
    const int W = s->image_width, H = s->image_height;
    const int64_t I = a->num_rendered;
    if (I < 0) return fail(BAGS_ERR_ARG, "num_rendered < 0");
    const int64_t cap = a->binning_capacity > 0 ? a->binning_capacity : I;     // what the forward carved the binning buffer for
    if (cap < I) return fail(BAGS_ERR_ARG, "binning_capacity %lld < num_rendered %lld", (long long)cap, (long long)I);
    if (!stt->binning || stt->binning_bytes < bags_binning_size(cap, W, H)) return fail(BAGS_ERR_SIZE, "binning buffer too small");
    if (!a->workspace || a->workspace_bytes < bags_backward_workspace_size(in->P, I)) return fail(BAGS_ERR_SIZE, "backward workspace too small");
    if (a->phase < BAGS_BWD_ALL || a->phase > BAGS_BWD_PREPROCESS) return fail(BAGS_ERR_ARG, "phase %d is not BAGS_BWD_ALL / _BLEND / _PREPROCESS", a->phase);
    if (a->grad_dldc && (!in->shs || in->colors_precomp || a->grad_shs || a->grad_shs_rest))
        return fail(BAGS_ERR_ARG, "grad_dldc (factored SH gradient) goes with inputs.shs and WITHOUT grad_shs / grad_shs_rest");
    if (in->shs_rest ? ((a->grad_shs != nullptr) != (a->grad_shs_rest != nullptr)) : (a->grad_shs_rest != nullptr))
        return fail(BAGS_ERR_ARG, "grad_shs_rest goes with inputs.shs_rest, and then grad_shs (features_dc) and grad_shs_rest are given together");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const StateViews v = bind_state(s, in, stt, cap);
    BwdWorkView w; carve_backward(a->workspace, in->P, I, &w);
    // the dense-scene mode (a byte per gradient record instead of zero records) is decided HERE, once: both launchers get the map or null
    const bool dense = I > 0 && bwd_dense_mode(I, cdiv(W, BAGS_TILE) * cdiv(H, BAGS_TILE), a->dense_per_tile);
    if (I > 0 && a->phase != BAGS_BWD_PREPROCESS) {
        // Profile mode 1 (bench.py's timed region: the dominant kernel's launch time for `roofline`): the start / stop events are attached
        // to the kernel's OWN dispatch (hipExtLaunchKernelGGL: the timestamps of its completion signal), not recorded around it.  Two
        // hipEventRecord calls are two more packets in the queue of a step whose seven launches otherwise follow each other without a
        // gap: they cost the timed region 10-25 us per step (0.605 against 0.594 ms on one device, 0.637 against 0.611 on the driver's
        // box of round 5), i.e. the measurement slowed down what it measured.
        hipEvent_t ea = nullptr, eb = nullptr;
        if (g_prof_mode == 1 && (g_prof_seq.fetch_add(1, std::memory_order_relaxed) % (unsigned long long)g_prof_stride) == 0ull) { ea = prof_event(); eb = prof_event(); }
        { ProfScope ps(ST_BLEND_BWD, st, true); HIP_TRY(launch_blend_bwd(*s, v.g, v.b, v.im, a->grad_color, w.partials, a->grad_means2D_densify != nullptr, v.binned, st,
                                                                  I, dense ? w.live_map : nullptr, w.live_bytes, ea, eb, grad_depth, grad_weights)); }
        if (ea) { std::lock_guard<std::mutex> lk(g_prof_mutex); g_prof_pending.push_back({ST_BLEND_BWD, ea, eb}); }
        DEBUG_SYNC(s, st, "blend_bwd");
    }
    if (a->phase == BAGS_BWD_BLEND) return BAGS_OK;          // the per-Gaussian half comes with a second call (BAGS_BWD_PREPROCESS)
    int nblocks = 0;
    { ProfScope ps(ST_PRE_BWD, st, true); HIP_TRY(launch_preprocess_bwd(*s, *in, v.g, w.partials, w.pose_slab, &nblocks, *a, st, v.binned, dense ? w.live_map : nullptr, extra)); }
    DEBUG_SYNC(s, st, "preprocess_bwd");
    { ProfScope ps(ST_POSE_REDUCE, st, true); HIP_TRY(launch_pose_reduce(w.pose_slab, nblocks, *a, st)); }
    DEBUG_SYNC(s, st, "pose_reduce");
    if (s->debug) {
        const size_t P = (size_t)in->P;
        const ScanItem items[] = {{"grad_means3D", a->grad_means3D, 3 * P}, {"grad_means2D", a->grad_means2D, 3 * P},
                                  {"grad_means2D_densify", a->grad_means2D_densify, 3 * P}, {"grad_shs", a->grad_shs, 3 * P * (size_t)(in->shs_rest ? 1 : s->sh_coeffs)},
                                  {"grad_shs_rest", in->shs_rest ? a->grad_shs_rest : nullptr, 3 * P * (size_t)(s->sh_coeffs - 1)},
                                  {"grad_colors_precomp", a->grad_colors_precomp, 3 * P}, {"grad_opacities", a->grad_opacities, P},
                                  {"grad_scales", a->grad_scales, 3 * P}, {"grad_rotations", a->grad_rotations, 4 * P},
                                  {"grad_cov3D_precomp", a->grad_cov3D_precomp, 6 * P}, {"grad_viewmatrix", a->grad_viewmatrix, 16},
                                  {"grad_projmatrix", a->grad_projmatrix, 16}, {"grad_intrinsic", a->grad_intrinsic, 16},
                                  {"grad_campos", a->grad_campos, 3}, {"grad_shift_factors", a->grad_shift_factors, 3}};
        return debug_scan(s, st, v.g.num_rendered + 8, items, 15, "the backward", fail);
    }
    return BAGS_OK;
}

int bags_sh_gradient_from_views(int32_t P, int32_t M, int32_t sh_degree, const float* means3D, const BagsShViews* views,
                                float* grad_shs, float* grad_shs_rest, int32_t accumulate, void* stream)
{
    if (P < 0) return fail(BAGS_ERR_ARG, "sh_gradient_from_views: P < 0");
    if (!views || views->n_views < 0 || views->n_views > BAGS_MAX_SH_VIEWS)
        return fail(BAGS_ERR_ARG, "sh_gradient_from_views: n_views must be 0..%d (more views: a second call with accumulate = 1)", BAGS_MAX_SH_VIEWS);
    if (sh_degree < 0 || sh_degree > 3 || M < 1 || (sh_degree + 1) * (sh_degree + 1) > M)
        return fail(BAGS_ERR_ARG, "sh_gradient_from_views: sh_degree %d needs %d coefficients, M = %d", sh_degree, (sh_degree + 1) * (sh_degree + 1), M);
    if (grad_shs_rest && M < 2) return fail(BAGS_ERR_ARG, "sh_gradient_from_views: grad_shs_rest needs M >= 2");
    if (P == 0 || views->n_views == 0) return BAGS_OK;
    if (!means3D || !grad_shs) return fail(BAGS_ERR_ARG, "sh_gradient_from_views: means3D / grad_shs must be given");
    for (int v = 0; v < views->n_views; ++v)
        if (!views->campos[v] || !views->dldc[v]) return fail(BAGS_ERR_ARG, "sh_gradient_from_views: view %d has a NULL campos / dldc", v);
    HIP_TRY(launch_sh_grad_from_views(P, M, sh_degree, means3D, *views, grad_shs, grad_shs_rest, accumulate, reinterpret_cast<hipStream_t>(stream)));
    return BAGS_OK;
}

int bags_debug_views(const BagsSettings* s, const BagsInputs* in, const BagsState* stt, int64_t I,
                     const BagsDebugViews* d, void* stream)
{
    int rc = check_common(s, in, stt);
    if (rc) return rc;
    if (!d) return fail(BAGS_ERR_ARG, "null views");
    const int W = s->image_width, H = s->image_height;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool lists = d->point_list || d->keys_sorted || d->ranges;          // the views that live in the binning buffer
    const StateViews v = bind_state(s, in, stt, lists ? (I > 0 ? I : 0) : -1);
    const GeomView& g = v.g; const BinView& b = v.b; const ImgView& im = v.im; const bool binned = v.binned;
    const size_t P = (size_t)in->P, T = (size_t)cdiv(W, BAGS_TILE) * cdiv(H, BAGS_TILE);
    if (d->tiles_touched && P) HIP_TRY(hipMemcpyAsync(d->tiles_touched, g.tiles_touched, P * 4, hipMemcpyDeviceToDevice, st));
    if (d->depth_bits && P) HIP_TRY(hipMemcpyAsync(d->depth_bits, g.depth_key, P * 4, hipMemcpyDeviceToDevice, st));
    if (d->rect && P) HIP_TRY(launch_unpack_rect(g.rect, in->P, d->rect, st));
    if (d->n_contrib) HIP_TRY(hipMemcpyAsync(d->n_contrib, im.n_contrib, (size_t)W * H * 4, hipMemcpyDeviceToDevice, st));
    if (d->final_T) HIP_TRY(hipMemcpyAsync(d->final_T, im.final_T, (size_t)W * H * 4, hipMemcpyDeviceToDevice, st));
    if (lists) {
        if (!stt->binning || stt->binning_bytes < bags_binning_size(I, W, H)) return fail(BAGS_ERR_SIZE, "binning buffer too small");
        const uint2* ranges = binned ? im.ranges : b.ranges;
        if (d->point_list && I) HIP_TRY(hipMemcpyAsync(d->point_list, b.point_list, (size_t)I * 4, hipMemcpyDeviceToDevice, st));
        if (d->keys_sorted && I) {
            if (binned) HIP_TRY(launch_debug_keys_ranges(ranges, b.point_list, g.depth_key, (int)T, d->keys_sorted, st));
            else HIP_TRY(launch_debug_keys(b.tile_sorted, b.point_list, g.depth_key, I, d->keys_sorted, st));
        }
        if (d->ranges) {
            if (in->P == 0 || (binned && I == 0 && in->P == 0)) HIP_TRY(hipMemsetAsync(d->ranges, 0, T * 8, st));
            else HIP_TRY(hipMemcpyAsync(d->ranges, ranges, T * 8, hipMemcpyDeviceToDevice, st));
        }
    }
    return BAGS_OK;
}

int bags_profile_enable(int mode)
{
    g_prof_mode = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
    return BAGS_OK;
}

int bags_profile_stride(int n)
{
    g_prof_stride = n < 1 ? 1 : n;
    g_prof_seq.store(0, std::memory_order_relaxed);
    return BAGS_OK;
}

int bags_profile_read(int max_stages, const char** names, double* total_ms, int64_t* calls)
{
    std::lock_guard<std::mutex> lk(g_prof_mutex);
    for (const ProfInterval& iv : g_prof_pending) {
        float ms = 0.f;
        if (hipEventSynchronize(iv.b) == hipSuccess && hipEventElapsedTime(&ms, iv.a, iv.b) == hipSuccess) {
            g_prof_ms[iv.stage] += ms; g_prof_calls[iv.stage] += 1;
        }
        g_prof_free.push_back(iv.a); g_prof_free.push_back(iv.b);
    }
    g_prof_pending.clear();
    const int n = max_stages < ST_COUNT ? max_stages : (int)ST_COUNT;
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = kStageNames[i];
        if (total_ms) total_ms[i] = g_prof_ms[i];
        if (calls) calls[i] = g_prof_calls[i];
    }
    for (int i = 0; i < ST_COUNT; ++i) { g_prof_ms[i] = 0.0; g_prof_calls[i] = 0; }
    return (int)ST_COUNT;
}

// ---------------------------------------------------------------------------------------------- photometric loss
size_t bags_loss_workspace_size(int32_t C, int32_t H, int32_t W)
{
    if (C <= 0 || H <= 0 || W <= 0) return 256;
    return loss_workspace_bytes(C, H, W);
}

int bags_loss_forward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, void* workspace,
                      size_t workspace_bytes, float* out_terms, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0) return fail(BAGS_ERR_ARG, "loss_forward: C, H, W must be positive (got %d, %d, %d)", C, H, W);
    if (!image || !gt || !workspace || !out_terms) return fail(BAGS_ERR_ARG, "loss_forward: null pointer");
    if (workspace_bytes < loss_workspace_bytes(C, H, W))
        return fail(BAGS_ERR_SIZE, "loss_forward: workspace %zu bytes < %zu", workspace_bytes, loss_workspace_bytes(C, H, W));
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return fail(BAGS_ERR_ARG, "loss_forward: the workspace is not 4-byte aligned");
    HIP_TRY(launch_loss_fwd(image, gt, C, H, W, workspace, out_terms, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_loss_backward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, const void* workspace,
                       size_t workspace_bytes, const float* grad_terms, float* grad_image, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0) return fail(BAGS_ERR_ARG, "loss_backward: C, H, W must be positive (got %d, %d, %d)", C, H, W);
    if (!image || !gt || !workspace || !grad_terms || !grad_image) return fail(BAGS_ERR_ARG, "loss_backward: null pointer");
    if (workspace_bytes < loss_workspace_bytes(C, H, W))
        return fail(BAGS_ERR_SIZE, "loss_backward: workspace %zu bytes < %zu", workspace_bytes, loss_workspace_bytes(C, H, W));
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return fail(BAGS_ERR_ARG, "loss_backward: the workspace is not 4-byte aligned");
    HIP_TRY(launch_loss_bwd(image, gt, C, H, W, workspace, grad_terms, grad_image, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_photometric_loss_forward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, void* workspace,
                                  size_t workspace_bytes, float lambda_dssim, float* out_loss_terms, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0) return fail(BAGS_ERR_ARG, "photometric_loss_forward: C, H, W must be positive (got %d, %d, %d)", C, H, W);
    if (!image || !gt || !workspace || !out_loss_terms) return fail(BAGS_ERR_ARG, "photometric_loss_forward: null pointer");
    if (!(lambda_dssim >= 0.f && lambda_dssim <= 1.f)) return fail(BAGS_ERR_ARG, "photometric_loss_forward: lambda_dssim %g outside [0, 1]", (double)lambda_dssim);
    if (workspace_bytes < loss_workspace_bytes(C, H, W))
        return fail(BAGS_ERR_SIZE, "photometric_loss_forward: workspace %zu bytes < %zu", workspace_bytes, loss_workspace_bytes(C, H, W));
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return fail(BAGS_ERR_ARG, "photometric_loss_forward: the workspace is not 4-byte aligned");
    HIP_TRY(launch_loss_fwd(image, gt, C, H, W, workspace, out_loss_terms, (hipStream_t)stream, true, lambda_dssim));
    return BAGS_OK;
}

int bags_photometric_loss_backward(const float* image, const float* gt, int32_t C, int32_t H, int32_t W, const void* workspace,
                                   size_t workspace_bytes, float lambda_dssim, const float* grad_loss, float* grad_image, void* stream)
{
    if (C <= 0 || H <= 0 || W <= 0) return fail(BAGS_ERR_ARG, "photometric_loss_backward: C, H, W must be positive (got %d, %d, %d)", C, H, W);
    if (!image || !gt || !workspace || !grad_loss || !grad_image) return fail(BAGS_ERR_ARG, "photometric_loss_backward: null pointer");
    if (!(lambda_dssim >= 0.f && lambda_dssim <= 1.f)) return fail(BAGS_ERR_ARG, "photometric_loss_backward: lambda_dssim %g outside [0, 1]", (double)lambda_dssim);
    if (workspace_bytes < loss_workspace_bytes(C, H, W))
        return fail(BAGS_ERR_SIZE, "photometric_loss_backward: workspace %zu bytes < %zu", workspace_bytes, loss_workspace_bytes(C, H, W));
    if (reinterpret_cast<uintptr_t>(workspace) % 4 != 0) return fail(BAGS_ERR_ARG, "photometric_loss_backward: the workspace is not 4-byte aligned");
    HIP_TRY(launch_loss_bwd(image, gt, C, H, W, workspace, grad_loss, grad_image, (hipStream_t)stream, true, lambda_dssim));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- camera chain
static int check_camera(const BagsCamera* c)
{
    if (!c) return fail(BAGS_ERR_ARG, "camera: null struct");
    if (!c->init_quaternion || !c->delta_quaternion || !c->init_translation || !c->delta_translation || !c->fovx || !c->fovy)
        return fail(BAGS_ERR_ARG, "camera: quaternion / translation / fov pointers must be given");
    if (!(c->zfar > c->znear) || !(c->znear > 0.f)) return fail(BAGS_ERR_ARG, "camera: need 0 < znear < zfar (got %g, %g)", c->znear, c->zfar);
    return BAGS_OK;
}

int bags_camera_forward(const BagsCamera* c, float* V, float* M, float* K, float* C, void* stream)
{
    int rc = check_camera(c);
    if (rc) return rc;
    if (!V || !M || !K || !C) return fail(BAGS_ERR_ARG, "camera_forward: null output");
    HIP_TRY(launch_camera_fwd(c->init_quaternion, c->delta_quaternion, c->init_translation, c->delta_translation, c->fovx, c->fovy,
                              c->global_rotation, c->global_translation_scale, c->znear, c->zfar, V, M, K, C, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_camera_backward(const BagsCamera* c, const float* gV, const float* gM, const float* gK, const float* gC,
                         float* g_dq, float* g_dt, float* g_fovx, float* g_fovy, float* g_grot, float* g_gscale, void* stream)
{
    int rc = check_camera(c);
    if (rc) return rc;
    HIP_TRY(launch_camera_bwd(c->init_quaternion, c->delta_quaternion, c->init_translation, c->delta_translation, c->fovx, c->fovy,
                              c->global_rotation, c->global_translation_scale, c->znear, c->zfar, gV, gM, gK, gC,
                              g_dq, g_dt, g_fovx, g_fovy, g_grot, g_gscale, (hipStream_t)stream));
    return BAGS_OK;
}

// the row list of a camera bank call (BagsPoseBank, BagsPoseAdamArgs): 1..BAGS_MAX_POSE_ROWS distinct rows, each in [0, N)
static int check_pose_rows(const char* op, int N, int n_rows, const int32_t* rows)
{
    if (N < 1) return fail(BAGS_ERR_ARG, "%s: N %d < 1", op, N);
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS) return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, n_rows, BAGS_MAX_POSE_ROWS);
    for (int v = 0; v < n_rows; ++v) {
        if (rows[v] < 0 || rows[v] >= N) return fail(BAGS_ERR_ARG, "%s: rows[%d] = %d is not in [0, %d)", op, v, rows[v], N);
        for (int u = 0; u < v; ++u)
            if (rows[u] == rows[v]) return fail(BAGS_ERR_ARG, "%s: row %d is listed twice (rows[%d] and rows[%d])", op, rows[v], u, v);
    }
    return BAGS_OK;
}

static int check_pose_bank(const char* op, const BagsPoseBank* b)
{
    if (!b) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (!b->init_quaternion || !b->init_translation || !b->near_far || !b->leaves)
        return fail(BAGS_ERR_ARG, "%s: init_quaternion / init_translation / near_far / leaves tables must be given", op);
    return check_pose_rows(op, b->N, b->n_rows, b->rows);
}

int bags_pose_bank_forward(const BagsPoseBank* b, float* V, float* M, float* K, float* C, void* stream)
{
    int rc = check_pose_bank("pose_bank_forward", b);
    if (rc) return rc;
    if (!V || !M || !K || !C) return fail(BAGS_ERR_ARG, "pose_bank_forward: null output");
    HIP_TRY(launch_pose_bank_fwd(*b, V, M, K, C, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_pose_bank_backward(const BagsPoseBank* b, const float* gV, const float* gM, const float* gK, const float* gC, float* grad_leaves,
                            float* g_grot, float* g_gscale, void* stream)
{
    int rc = check_pose_bank("pose_bank_backward", b);
    if (rc) return rc;
    if (!grad_leaves) return fail(BAGS_ERR_ARG, "pose_bank_backward: null grad_leaves");
    if (grad_leaves == b->leaves) return fail(BAGS_ERR_ARG, "pose_bank_backward: grad_leaves must not be the leaves table");
    if (g_grot && !b->global_rotation) return fail(BAGS_ERR_ARG, "pose_bank_backward: g_global_rotation asked for without a global_rotation");
    if (g_gscale && !b->global_translation_scale)
        return fail(BAGS_ERR_ARG, "pose_bank_backward: g_global_translation_scale asked for without a global_translation_scale");
    HIP_TRY(launch_pose_bank_bwd(*b, gV, gM, gK, gC, grad_leaves, g_grot, g_gscale, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- distortion resampling
static int check_resample(int C, int H, int W, int h, int w, int Hf, int Wf, int Hc, int Wc)
{
    if (C <= 0 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || Hf <= 0 || Wf <= 0 || Hc <= 0 || Wc <= 0)
        return fail(BAGS_ERR_ARG, "resample: every extent must be positive");
    if (Hc > Hf || Wc > Wf) return fail(BAGS_ERR_ARG, "resample: crop %dx%d exceeds the flow size %dx%d", Wc, Hc, Wf, Hf);
    // the backward keeps a 16x16xC accumulator of 64-bit words in LDS (2 KB per channel)
    if (C > 24) return fail(BAGS_ERR_ARG, "resample: at most 24 channels per call (got %d): split the image along C", C);
    if (H > 32000 || W > 32000) return fail(BAGS_ERR_ARG, "resample: image %dx%d too large (tap coordinates are kept as int16)", W, H);
    return BAGS_OK;
}

int bags_resample_forward(const float* image, int32_t C, int32_t H, int32_t W, const float* ctrl, int32_t h, int32_t w,
                          int32_t Hf, int32_t Wf, int32_t Hc, int32_t Wc, float* out, float* mask, float* flow_out, void* stream)
{
    int rc = check_resample(C, H, W, h, w, Hf, Wf, Hc, Wc);
    if (rc) return rc;
    if (!image || !ctrl || !out) return fail(BAGS_ERR_ARG, "resample_forward: null pointer");
    HIP_TRY(launch_resample_fwd(image, C, H, W, ctrl, h, w, Hf, Wf, Hc, Wc, out, mask, flow_out, (hipStream_t)stream));
    return BAGS_OK;
}

size_t bags_resample_workspace_size(int32_t H, int32_t W, int32_t Hc, int32_t Wc)
{
    return resample_workspace_bytes(H > 0 ? H : 1, W > 0 ? W : 1, Hc > 0 ? Hc : 1, Wc > 0 ? Wc : 1);
}

int bags_resample_backward(const float* image, int32_t C, int32_t H, int32_t W, const float* ctrl, int32_t h, int32_t w,
                           int32_t Hf, int32_t Wf, int32_t Hc, int32_t Wc, const float* grad_out, void* workspace,
                           size_t workspace_bytes, float* grad_image, float* grad_ctrl, void* stream)
{
    int rc = check_resample(C, H, W, h, w, Hf, Wf, Hc, Wc);
    if (rc) return rc;
    if (!image || !ctrl || !grad_out) return fail(BAGS_ERR_ARG, "resample_backward: null pointer");
    if (!grad_image && !grad_ctrl) return BAGS_OK;
    if (!workspace || workspace_bytes < resample_workspace_bytes(H, W, Hc, Wc))
        return fail(BAGS_ERR_SIZE, "resample_backward: needs a workspace of %zu bytes", resample_workspace_bytes(H, W, Hc, Wc));
    HIP_TRY(launch_resample_bwd(image, C, H, W, ctrl, h, w, Hf, Wf, Hc, Wc, grad_out, workspace, grad_image, grad_ctrl, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- cubemap stitch
static int check_faces(const char* who, const BagsFaces* f, int h, int w, int Hf, int Wf, int Hc, int Wc)
{
    if (!f) return fail(BAGS_ERR_ARG, "%s: null BagsFaces", who);
    if (f->n_faces < 1 || f->n_faces > BAGS_MAX_FACES)
        return fail(BAGS_ERR_ARG, "%s: n_faces %d outside 1..%d", who, f->n_faces, BAGS_MAX_FACES);
    if (f->C <= 0 || f->H <= 0 || f->W <= 0 || h <= 0 || w <= 0 || Hf <= 0 || Wf <= 0 || Hc <= 0 || Wc <= 0)
        return fail(BAGS_ERR_ARG, "%s: every extent must be positive", who);
    if (f->C > 4) return fail(BAGS_ERR_ARG, "%s: at most 4 channels per face (got %d)", who, f->C);
    if (Hc > Hf || Wc > Wf) return fail(BAGS_ERR_ARG, "%s: crop %dx%d exceeds the flow size %dx%d", who, Wc, Hc, Wf, Hf);
    if (f->H > 32000 || f->W > 32000) return fail(BAGS_ERR_ARG, "%s: face %dx%d too large (tap coordinates are kept as int16)", who, f->W, f->H);
    for (int i = 0; i < f->n_faces; ++i)
        if (!f->image[i]) return fail(BAGS_ERR_ARG, "%s: null image of face %d", who, i);
    return BAGS_OK;
}

size_t bags_resample_faces_workspace_size(int32_t n_faces, int32_t H, int32_t W, int32_t Hc, int32_t Wc)
{
    if (n_faces < 1 || n_faces > BAGS_MAX_FACES || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0) return 0;
    return resample_faces_workspace_bytes(n_faces, H, W, Hc, Wc);
}

int bags_resample_faces_forward(const BagsFaces* f, const float* ctrl, int32_t h, int32_t w, int32_t Hf, int32_t Wf, int32_t Hc, int32_t Wc,
                                float* out, int8_t* face_index, void* stream)
{
    int rc = check_faces("resample_faces_forward", f, h, w, Hf, Wf, Hc, Wc);
    if (rc) return rc;
    if (!ctrl || !out || !face_index) return fail(BAGS_ERR_ARG, "resample_faces_forward: null pointer");
    HIP_TRY(launch_resample_faces_fwd(*f, ctrl, h, w, Hf, Wf, Hc, Wc, out, face_index, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_resample_faces_backward(const BagsFaces* f, const float* ctrl, int32_t h, int32_t w, int32_t Hf, int32_t Wf, int32_t Hc, int32_t Wc,
                                 const int8_t* face_index, const float* grad_out, void* workspace, size_t workspace_bytes,
                                 float* const grad_faces[BAGS_MAX_FACES], float* grad_ctrl, void* stream)
{
    int rc = check_faces("resample_faces_backward", f, h, w, Hf, Wf, Hc, Wc);
    if (rc) return rc;
    if (!ctrl || !face_index || !grad_out) return fail(BAGS_ERR_ARG, "resample_faces_backward: null pointer");
    bool any = grad_ctrl != nullptr;
    for (int i = 0; grad_faces && i < f->n_faces; ++i) any |= grad_faces[i] != nullptr;
    if (!any) return BAGS_OK;
    const size_t need = resample_faces_workspace_bytes(f->n_faces, f->H, f->W, Hc, Wc);
    if (!workspace || workspace_bytes < need) return fail(BAGS_ERR_SIZE, "resample_faces_backward: needs a workspace of %zu bytes", need);
    HIP_TRY(launch_resample_faces_bwd(*f, ctrl, h, w, Hf, Wf, Hc, Wc, face_index, grad_out, workspace, grad_faces, grad_ctrl, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- activations
static int check_raw(const BagsRawGaussians* r, bool features)      // features: the SH concatenation (or its gradient) is asked for
{
    if (!r) return fail(BAGS_ERR_ARG, "activations: null struct");
    if (r->P < 0 || r->K < 1) return fail(BAGS_ERR_ARG, "activations: need P >= 0 and K >= 1 (got %d, %d)", r->P, r->K);
    if (r->P > 0 && (!r->opacity || !r->scaling || !r->rotation)) return fail(BAGS_ERR_ARG, "activations: null parameter pointer");
    if (r->P > 0 && features && (!r->features_dc || (r->K > 1 && !r->features_rest)))
        return fail(BAGS_ERR_ARG, "activations: null feature pointer (features_dc / features_rest may only be NULL when shs / g_shs is)");
    return BAGS_OK;
}

int bags_activations_forward(const BagsRawGaussians* r, float* shs, float* opacity, float* scales, float* rotations, void* stream)
{
    int rc = check_raw(r, shs != nullptr);
    if (rc) return rc;
    HIP_TRY(launch_activations_fwd(r->P, r->K, r->features_dc, r->features_rest, r->opacity, r->scaling, r->rotation, shs, opacity,
                                   scales, rotations, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_activations_backward(const BagsRawGaussians* r, const float* g_shs, const float* g_opacity, const float* g_scales,
                              const float* g_rotations, float* g_dc, float* g_rest, float* g_opacity_raw, float* g_scaling,
                              float* g_rotation, void* stream)
{
    int rc = check_raw(r, g_shs != nullptr && (g_dc != nullptr || g_rest != nullptr));
    if (rc) return rc;
    HIP_TRY(launch_activations_bwd(r->P, r->K, r->features_dc, r->features_rest, r->opacity, r->scaling, r->rotation, g_shs, g_opacity,
                                   g_scales, g_rotations, g_dc, g_rest, g_opacity_raw, g_scaling, g_rotation, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_activations_filtered_forward(const BagsRawGaussians* r, const float* filter_3D, float* shs, float* opacity, float* scales,
                                      float* rotations, void* stream)
{
    int rc = check_raw(r, shs != nullptr);
    if (rc) return rc;
    if (r->P > 0 && !filter_3D) return fail(BAGS_ERR_ARG, "activations_filtered_forward: NULL filter_3D");
    HIP_TRY(launch_activations_fwd(r->P, r->K, r->features_dc, r->features_rest, r->opacity, r->scaling, r->rotation, shs, opacity,
                                   scales, rotations, (hipStream_t)stream, filter_3D));
    return BAGS_OK;
}

int bags_activations_filtered_backward(const BagsRawGaussians* r, const float* filter_3D, const float* g_shs, const float* g_opacity,
                                       const float* g_scales, const float* g_rotations, float* g_dc, float* g_rest, float* g_opacity_raw,
                                       float* g_scaling, float* g_rotation, void* stream)
{
    int rc = check_raw(r, g_shs != nullptr && (g_dc != nullptr || g_rest != nullptr));
    if (rc) return rc;
    if (r->P > 0 && !filter_3D) return fail(BAGS_ERR_ARG, "activations_filtered_backward: NULL filter_3D");
    HIP_TRY(launch_activations_bwd(r->P, r->K, r->features_dc, r->features_rest, r->opacity, r->scaling, r->rotation, g_shs, g_opacity,
                                   g_scales, g_rotations, g_dc, g_rest, g_opacity_raw, g_scaling, g_rotation, (hipStream_t)stream, filter_3D));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- SH colours
static int check_sh_colors(const BagsShColors* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "sh_colors: null struct");
    if (a->P < 0) return fail(BAGS_ERR_ARG, "sh_colors: P < 0 (got %d)", a->P);
    if (a->sh_degree < 0 || a->sh_degree > 3) return fail(BAGS_ERR_ARG, "sh_colors: sh_degree %d not in 0..3", a->sh_degree);
    if (a->K != 1 && a->K != 4 && a->K != 9 && a->K != 16) return fail(BAGS_ERR_ARG, "sh_colors: K %d not one of 1, 4, 9, 16", a->K);
    if ((a->sh_degree + 1) * (a->sh_degree + 1) > a->K)
        return fail(BAGS_ERR_ARG, "sh_colors: sh_degree %d needs %d coefficients, K is %d", a->sh_degree, (a->sh_degree + 1) * (a->sh_degree + 1), a->K);
    if (a->shs_rest && a->K < 4) return fail(BAGS_ERR_ARG, "sh_colors: shs_rest needs K >= 4 (got %d)", a->K);
    if (a->P > 0 && (!a->shs || !a->xyz || !a->campos)) return fail(BAGS_ERR_ARG, "sh_colors: shs / xyz / campos must be given");
    if (!a->shs_rest && a->K == 16 && (reinterpret_cast<size_t>(a->shs) & 15))
        return fail(BAGS_ERR_ARG, "sh_colors: packed shs (P,16,3) must be 16-byte aligned");
    return BAGS_OK;
}

// The gradient arguments of a backward entry point, `op` its name, `null_rgb` what it says of a missing grad_rgb.  want_campos:
// some dL/dcampos is asked for, so the workspace must hold the slab of V views, which *slab then is.
static int check_sh_grads(const char* op, const char* null_rgb, int P, bool split, int V, const void* grad_rgb, const float* grad_shs,
                          const float* grad_shs_rest, bool want_campos, void* workspace, size_t workspace_bytes, float** slab)
{
    if (P > 0 && !grad_rgb) return fail(BAGS_ERR_ARG, "%s_backward: %s", op, null_rgb);
    if (grad_shs_rest && !split) return fail(BAGS_ERR_ARG, "%s_backward: grad_shs_rest without shs_rest", op);
    if ((reinterpret_cast<size_t>(grad_shs) | reinterpret_cast<size_t>(grad_shs_rest)) & 15)
        return fail(BAGS_ERR_ARG, "%s_backward: grad_shs / grad_shs_rest must be 16-byte aligned", op);
    if (want_campos) {
        const size_t need = carve_sh_colors(nullptr, P, V, nullptr) + BASE_SLACK;
        if (!workspace || workspace_bytes < need) return fail(BAGS_ERR_SIZE, "%s_backward: grad_campos needs a workspace of %zu bytes", op, need);
        carve_sh_colors(workspace, P, V, slab);
    }
    return BAGS_OK;
}

size_t bags_sh_colors_workspace_size(int32_t P) { return carve_sh_colors(nullptr, P, 1, nullptr) + BASE_SLACK; }

int bags_sh_colors_forward(const BagsShColors* a, float* rgb, void* stream)
{
    int rc = check_sh_colors(a);
    if (rc) return rc;
    if (a->P == 0) return BAGS_OK;
    if (!rgb) return fail(BAGS_ERR_ARG, "sh_colors_forward: null rgb");
    HIP_TRY(launch_sh_colors_fwd(*a, rgb, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_sh_colors_backward(const BagsShColors* a, const float* grad_rgb, void* workspace, size_t workspace_bytes, float* grad_shs,
                            float* grad_shs_rest, float* grad_xyz, float* grad_campos, void* stream)
{
    int rc = check_sh_colors(a);
    if (rc) return rc;
    if (!grad_shs && !grad_shs_rest && !grad_xyz && !grad_campos) return BAGS_OK;
    float* slab = nullptr;
    rc = check_sh_grads("sh_colors", "null grad_rgb", a->P, a->shs_rest != nullptr, 1, grad_rgb, grad_shs, grad_shs_rest, grad_campos != nullptr, workspace, workspace_bytes, &slab);
    if (rc) return rc;
    HIP_TRY(launch_sh_colors_bwd(*a, grad_rgb, slab, grad_shs, grad_shs_rest, grad_xyz, grad_campos, (hipStream_t)stream));
    return BAGS_OK;
}

// the V views of one step: the single-view rules for everything the views share, then the table
static int check_sh_colors_views(const BagsShColorsViews* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "sh_colors_views: null struct");
    if (a->V < 1 || a->V > BAGS_MAX_SH_VIEWS)
        return fail(BAGS_ERR_ARG, "sh_colors_views: V %d not in 1..%d (more views: one call per chunk)", a->V, BAGS_MAX_SH_VIEWS);
    const BagsShColors one{a->P, a->K, a->sh_degree, 0, a->shs, a->shs_rest, a->xyz, a->campos[0]};
    int rc = check_sh_colors(&one);
    if (rc) return rc;
    for (int v = 0; a->P > 0 && v < a->V; ++v)
        if (!a->campos[v]) return fail(BAGS_ERR_ARG, "sh_colors_views: campos[%d] is NULL (V = %d)", v, a->V);
    return BAGS_OK;
}

size_t bags_sh_colors_views_workspace_size(int32_t P, int32_t V) { return carve_sh_colors(nullptr, P, V, nullptr) + BASE_SLACK; }

int bags_sh_colors_views_forward(const BagsShColorsViews* a, float* const rgb[], void* stream)
{
    int rc = check_sh_colors_views(a);
    if (rc) return rc;
    if (a->P == 0) return BAGS_OK;
    if (!rgb) return fail(BAGS_ERR_ARG, "sh_colors_views_forward: null rgb table");
    for (int v = 0; v < a->V; ++v)
        if (!rgb[v]) return fail(BAGS_ERR_ARG, "sh_colors_views_forward: rgb[%d] is NULL (V = %d)", v, a->V);
    HIP_TRY(launch_sh_colors_views_fwd(*a, rgb, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_sh_colors_views_backward(const BagsShColorsViews* a, const float* const grad_rgb[], void* workspace, size_t workspace_bytes,
                                  float* grad_shs, float* grad_shs_rest, float* grad_xyz, float* const grad_campos[], void* stream)
{
    int rc = check_sh_colors_views(a);
    if (rc) return rc;
    bool any_campos = false;
    for (int v = 0; grad_campos && v < a->V; ++v) any_campos = any_campos || grad_campos[v] != nullptr;
    if (!grad_shs && !grad_shs_rest && !grad_xyz && !any_campos) return BAGS_OK;
    float* slab = nullptr;
    rc = check_sh_grads("sh_colors_views", "null grad_rgb table (its entries may be NULL, the table not)", a->P, a->shs_rest != nullptr, a->V, grad_rgb,
                        grad_shs, grad_shs_rest, any_campos, workspace, workspace_bytes, &slab);
    if (rc) return rc;
    HIP_TRY(launch_sh_colors_views_bwd(*a, grad_rgb, slab, grad_shs, grad_shs_rest, grad_xyz, any_campos ? grad_campos : nullptr, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- optimizer step
int bags_adam_step(const BagsAdamArgs* a, const BagsDensifyStats* stats, void* stream)
{
    if (!a) return fail(BAGS_ERR_ARG, "adam: null struct");
    if (a->P < 0) return fail(BAGS_ERR_ARG, "adam: P < 0 (got %d)", a->P);
    if (a->n_groups < 1 || a->n_groups > BAGS_ADAM_MAX_GROUPS)
        return fail(BAGS_ERR_ARG, "adam: n_groups %d not in 1..%d", a->n_groups, BAGS_ADAM_MAX_GROUPS);
    for (int k = 0; k < a->n_groups; ++k) {
        const BagsAdamGroup& g = a->groups[k];
        if (g.width <= 0) return fail(BAGS_ERR_ARG, "adam: group %d: width %d <= 0", k, g.width);
        if (g.grad && (!g.param || !g.exp_avg || !g.exp_avg_sq))
            return fail(BAGS_ERR_ARG, "adam: group %d has a grad but a NULL param / exp_avg / exp_avg_sq", k);
    }
    if (stats) {
        const int given = (stats->radii != nullptr) + (stats->grad_means2D != nullptr) + (stats->xyz_gradient_accum != nullptr) +
                          (stats->denom != nullptr) + (stats->max_radii2D != nullptr);
        if (given != 0 && given != 5)
            return fail(BAGS_ERR_ARG, "adam: stats block needs all of radii, grad_means2D, xyz_gradient_accum, denom, max_radii2D or none (%d of 5 given)", given);
        if (given == 5 && stats->grad_stride < 2) return fail(BAGS_ERR_ARG, "adam: stats grad_stride %d < 2", stats->grad_stride);
    }
    if (a->P == 0) return BAGS_OK;
    HIP_TRY(launch_adam(*a, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_pose_adam_step(const BagsPoseAdamArgs* a, void* stream)
{
    if (!a) return fail(BAGS_ERR_ARG, "pose_adam: null struct");
    if (!a->leaves || !a->grad || !a->exp_avg || !a->exp_avg_sq) return fail(BAGS_ERR_ARG, "pose_adam: leaves / grad / exp_avg / exp_avg_sq tables must be given");
    int rc = check_pose_rows("pose_adam", a->N, a->n_rows, a->rows);
    if (rc) return rc;
    HIP_TRY(launch_pose_adam(*a, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- densify-and-prune, opacity reset
size_t bags_densify_workspace_size(int32_t P) { return densify_workspace_bytes(P); }

static int check_densify_rule(const BagsDensifyRule* r, const void* workspace, size_t workspace_bytes)
{
    if (!r) return fail(BAGS_ERR_ARG, "densify: null rule");
    if (r->P < 0) return fail(BAGS_ERR_ARG, "densify: P < 0 (got %d)", r->P);
    if (r->N < 1 || r->N > BAGS_DENSIFY_MAX_CHILDREN) return fail(BAGS_ERR_ARG, "densify: N %d not in 1..%d", r->N, BAGS_DENSIFY_MAX_CHILDREN);
    if (r->screen_size_mode != BAGS_SCREEN_PUBLISHED && r->screen_size_mode != BAGS_SCREEN_PRE_DENSIFY)
        return fail(BAGS_ERR_ARG, "densify: screen_size_mode %d is neither BAGS_SCREEN_PUBLISHED nor BAGS_SCREEN_PRE_DENSIFY", r->screen_size_mode);
    if (r->use_screen_size != 0 && r->use_screen_size != 1) return fail(BAGS_ERR_ARG, "densify: use_screen_size %d is not 0 or 1", r->use_screen_size);
    if (!(r->max_grad == r->max_grad) || !(r->min_opacity == r->min_opacity) || !(r->dense_threshold == r->dense_threshold))
        return fail(BAGS_ERR_ARG, "densify: max_grad / min_opacity / dense_threshold is NaN");
    if (r->use_screen_size && (!(r->world_threshold == r->world_threshold) || !(r->max_screen_size == r->max_screen_size)))
        return fail(BAGS_ERR_ARG, "densify: world_threshold / max_screen_size is NaN");
    if (r->P == 0) return BAGS_OK;
    if (!r->xyz_gradient_accum) return fail(BAGS_ERR_ARG, "densify: NULL xyz_gradient_accum");
    if (!r->denom) return fail(BAGS_ERR_ARG, "densify: NULL denom");
    if (!r->max_radii2D) return fail(BAGS_ERR_ARG, "densify: NULL max_radii2D");
    if (!r->scaling) return fail(BAGS_ERR_ARG, "densify: NULL scaling");
    if (!r->opacity) return fail(BAGS_ERR_ARG, "densify: NULL opacity");
    if (!workspace) return fail(BAGS_ERR_ARG, "densify: NULL workspace");
    if (workspace_bytes < densify_workspace_bytes(r->P))
        return fail(BAGS_ERR_SIZE, "densify: workspace %zu bytes < %zu", workspace_bytes, densify_workspace_bytes(r->P));
    return BAGS_OK;
}

int bags_densify_plan(const BagsDensifyRule* r, void* workspace, size_t workspace_bytes, int64_t* host_counts, void* stream)
{
    if (const int rc = check_densify_rule(r, workspace, workspace_bytes)) return rc;
    if (!host_counts) return fail(BAGS_ERR_ARG, "densify: NULL host_counts");
    for (int k = 0; k < BAGS_DENSIFY_COUNTS; ++k) host_counts[k] = 0;
    if (r->P == 0) return BAGS_OK;
    u32 t[5] = {0, 0, 0, 0, 0};                      // kept, clones out, split rows out, clone-selected, split-selected
    HIP_TRY(launch_densify_plan(*r, workspace, t, (hipStream_t)stream));
    const int64_t children = (int64_t)t[2] * r->N, P_new = (int64_t)t[0] + t[1] + children;
    host_counts[BAGS_COUNT_KEPT] = t[0];
    host_counts[BAGS_COUNT_CLONES] = t[3];
    host_counts[BAGS_COUNT_SPLIT] = t[4];
    host_counts[BAGS_COUNT_PRUNED] = (int64_t)r->P + t[3] + (int64_t)t[4] * (r->N - 1) - P_new;
    host_counts[BAGS_COUNT_P_NEW] = P_new;
    host_counts[BAGS_COUNT_CLONES_OUT] = t[1];
    host_counts[BAGS_COUNT_CHILDREN_OUT] = children;
    if (P_new > 0x7FFFFFFFll) return fail(BAGS_ERR_SIZE, "densify: the new set would hold %lld rows (> 2^31 - 1)", (long long)P_new);
    return BAGS_OK;
}

static inline bool misaligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15u) != 0; }

// What bags_densify_apply and the MCMC entry points both ask of their groups and of a resized set's outputs; the callers keep their order.
static int check_group_count(const char* op, const void* groups, int32_t n_groups)
{
    if (n_groups < 1 || n_groups > BAGS_DENSIFY_MAX_GROUPS) return fail(BAGS_ERR_ARG, "%s: n_groups %d not in 1..%d", op, n_groups, BAGS_DENSIFY_MAX_GROUPS);
    if (!groups) return fail(BAGS_ERR_ARG, "%s: NULL groups", op);
    return BAGS_OK;
}

static int check_group_shape(const char* op, int k, int32_t width, int32_t role)
{
    if (width <= 0) return fail(BAGS_ERR_ARG, "%s: group %d: width %d <= 0", op, k, width);
    if (role < BAGS_ROLE_OTHER || role > BAGS_ROLE_OPACITY) return fail(BAGS_ERR_ARG, "%s: group %d: unknown role %d", op, k, role);
    const int want = role == BAGS_ROLE_XYZ || role == BAGS_ROLE_SCALING ? 3 : role == BAGS_ROLE_ROTATION ? 4 : role == BAGS_ROLE_OPACITY ? 1 : width;
    if (width != want) return fail(BAGS_ERR_ARG, "%s: group %d: width %d, but its role %d has width %d", op, k, width, role, want);
    return BAGS_OK;
}

static int check_group_aligned(const char* op, int k, const float* param_out, const float* exp_avg_out, const float* exp_avg_sq_out)
{
    if (misaligned16(param_out) || misaligned16(exp_avg_out) || misaligned16(exp_avg_sq_out))
        return fail(BAGS_ERR_ARG, "%s: group %d: param_out / exp_avg_out / exp_avg_sq_out is not 16-byte aligned", op, k);
    return BAGS_OK;
}

static int check_stats_out(const char* op, const float* accum_out, const float* denom_out, const float* radii_out)
{
    if (!accum_out || !denom_out || !radii_out) return fail(BAGS_ERR_ARG, "%s: NULL xyz_gradient_accum_out / denom_out / max_radii2D_out", op);
    if (misaligned16(accum_out) || misaligned16(denom_out) || misaligned16(radii_out))
        return fail(BAGS_ERR_ARG, "%s: xyz_gradient_accum_out / denom_out / max_radii2D_out is not 16-byte aligned", op);
    return BAGS_OK;
}

int bags_densify_apply(const BagsDensifyRule* r, const BagsDensifyGroup* groups, int32_t n_groups, void* workspace, size_t workspace_bytes,
                       int64_t P_new, float* accum_out, float* denom_out, float* radii_out, int32_t* provenance, void* stream)
{
    if (const int rc = check_densify_rule(r, workspace, workspace_bytes)) return rc;
    if (const int rc = check_group_count("densify", groups, n_groups)) return rc;
    if (P_new < 0 || P_new > (int64_t)r->P * (r->N > 2 ? r->N : 2))
        return fail(BAGS_ERR_ARG, "densify: P_new %lld not in 0..P * max(2, N)", (long long)P_new);
    int n_xyz = 0, n_scaling = 0, n_rotation = 0;
    for (int k = 0; k < n_groups; ++k) {
        const BagsDensifyGroup& g = groups[k];
        if (const int rc = check_group_shape("densify", k, g.width, g.role)) return rc;
        n_xyz += g.role == BAGS_ROLE_XYZ; n_scaling += g.role == BAGS_ROLE_SCALING; n_rotation += g.role == BAGS_ROLE_ROTATION;
        if (r->P > 0 && P_new > 0) {
            const int moments = (g.exp_avg != nullptr) + (g.exp_avg_sq != nullptr) + (g.exp_avg_out != nullptr) + (g.exp_avg_sq_out != nullptr);
            if (moments != 0 && moments != 4)
                return fail(BAGS_ERR_ARG, "densify: group %d: exp_avg, exp_avg_sq and their outputs are given together or not at all (%d of 4 given)", k, moments);
            if (!g.param || !g.param_out) return fail(BAGS_ERR_ARG, "densify: group %d: NULL param / param_out", k);
            if (const int rc = check_group_aligned("densify", k, g.param_out, g.exp_avg_out, g.exp_avg_sq_out)) return rc;
        }
    }
    if (n_xyz != 1 || n_scaling != 1 || n_rotation != 1)
        return fail(BAGS_ERR_ARG, "densify: role xyz, scaling and rotation must each be given once (got %d, %d, %d)", n_xyz, n_scaling, n_rotation);
    if (r->P == 0 || P_new == 0) return BAGS_OK;
    if (const int rc = check_stats_out("densify", accum_out, denom_out, radii_out)) return rc;
    if (!provenance) return fail(BAGS_ERR_ARG, "densify: NULL provenance (it is the gather index of the copy)");
    if (misaligned16(provenance)) return fail(BAGS_ERR_ARG, "densify: provenance is not 16-byte aligned");
    HIP_TRY(launch_densify_apply(*r, groups, n_groups, workspace, (long long)P_new, accum_out, denom_out, radii_out, provenance, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_reset_opacity(float* opacity, float* exp_avg, float* exp_avg_sq, int32_t P, void* stream)
{
    if (P < 0) return fail(BAGS_ERR_ARG, "reset_opacity: P < 0 (got %d)", P);
    if (P == 0) return BAGS_OK;
    if (!opacity) return fail(BAGS_ERR_ARG, "reset_opacity: NULL opacity");
    HIP_TRY(launch_reset_opacity(opacity, exp_avg, exp_avg_sq, P, 0.01f, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- lens network
#define LENS_TORCH_PATH "a larger net is a GEMM problem, not a launch-count one: use the PyTorch path, lens_field_torch"
static const int64_t LENS_MAX_POINTS = (int64_t)1 << 36;       // tiles of 64 points fit the grid's 31 bits

static bool lens_shape_ok(int B, int H, int n)
{
    return B >= 1 && B <= BAGS_LENS_MAX_BLOCKS && H >= 1 && H <= BAGS_LENS_MAX_HIDDEN && n >= 0 && n <= BAGS_LENS_MAX_INTERNAL_LAYERS;
}

static int check_lens_field(const char* op, const BagsLensField* a, int64_t M)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (!lens_shape_ok(a->blocks, a->hidden, a->internal_layers))
        return fail(BAGS_ERR_ARG, "%s: blocks %d, hidden %d, internal_layers %d not in 1..%d, 1..%d, 0..%d (" LENS_TORCH_PATH ")", op, a->blocks, a->hidden,
                    a->internal_layers, BAGS_LENS_MAX_BLOCKS, BAGS_LENS_MAX_HIDDEN, BAGS_LENS_MAX_INTERNAL_LAYERS);
    if (M < 0 || M > LENS_MAX_POINTS) return fail(BAGS_ERR_ARG, "%s: M %lld not in 0..2^36", op, (long long)M);
    if (!a->params) return fail(BAGS_ERR_ARG, "%s: null params", op);
    return BAGS_OK;
}

// 0 for a shape outside the limits (the entry points refuse it) or M < 0
size_t bags_lens_field_workspace_size(int32_t blocks, int32_t hidden, int32_t internal_layers, int64_t M)
{
    if (!lens_shape_ok(blocks, hidden, internal_layers) || M < 0 || M > LENS_MAX_POINTS) return 0;
    return lens_field_workspace_bytes(blocks, hidden, internal_layers, M);
}

int bags_lens_field_forward(const BagsLensField* a, const float* x, int64_t M, float* y, void* stream)
{
    if (const int rc = check_lens_field("lens_field_forward", a, M)) return rc;
    if (M == 0) return BAGS_OK;
    if (!x || !y) return fail(BAGS_ERR_ARG, "lens_field_forward: null x / y");
    HIP_TRY(launch_lens_field_fwd(*a, x, M, y, false, 0, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_lens_field_inverse(const BagsLensField* a, const float* y, int64_t M, int32_t iterations, float* x, void* stream)
{
    if (const int rc = check_lens_field("lens_field_inverse", a, M)) return rc;
    if (iterations < 0) return fail(BAGS_ERR_ARG, "lens_field_inverse: iterations %d < 0", iterations);
    if (M == 0) return BAGS_OK;
    if (!x || !y) return fail(BAGS_ERR_ARG, "lens_field_inverse: null y / x");
    HIP_TRY(launch_lens_field_fwd(*a, y, M, x, true, iterations, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_lens_field_backward(const BagsLensField* a, const float* x, int64_t M, const float* grad_y, void* workspace, size_t workspace_bytes,
                             float* grad_x, float* grad_params, void* stream)
{
    if (const int rc = check_lens_field("lens_field_backward", a, M)) return rc;
    if (!grad_x && !grad_params) return BAGS_OK;
    if (M == 0) {
        if (grad_params)
            HIP_TRY(hipMemsetAsync(grad_params, 0, (size_t)a->blocks * lens_block_floats(a->hidden, a->internal_layers) * sizeof(float), (hipStream_t)stream));
        return BAGS_OK;
    }
    if (!x || !grad_y) return fail(BAGS_ERR_ARG, "lens_field_backward: null x / grad_y");
    if (grad_params == a->params) return fail(BAGS_ERR_ARG, "lens_field_backward: grad_params must not be the params vector");
    const size_t need = lens_field_workspace_bytes(a->blocks, a->hidden, a->internal_layers, M);
    if (!workspace || workspace_bytes < need) return fail(BAGS_ERR_SIZE, "lens_field_backward: needs a workspace of %zu bytes", need);
    HIP_TRY(launch_lens_field_bwd(*a, x, M, grad_y, workspace, grad_x, grad_params, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- kNN scale initialiser
size_t bags_knn_workspace_size(int32_t P) { return knn_workspace_bytes(P > 0 ? P : 1); }

int bags_knn_mean_dist2(const float* points, int32_t P, void* workspace, size_t workspace_bytes, float* out, void* stream)
{
    if (P < 0) return fail(BAGS_ERR_ARG, "knn: P < 0");
    if (P == 0) return BAGS_OK;
    if (!points || !workspace || !out) return fail(BAGS_ERR_ARG, "knn: null pointer");
    if (workspace_bytes < knn_workspace_bytes(P))
        return fail(BAGS_ERR_SIZE, "knn: workspace %zu bytes < %zu", workspace_bytes, knn_workspace_bytes(P));
    HIP_TRY(launch_knn(points, P, workspace, out, (hipStream_t)stream));
    return BAGS_OK;
}

// ---------------------------------------------------------------------------------------------- MCMC relocation, growth and noise
static int check_binoms(const char* op, const float* binoms, int32_t n_max)
{
    if (!binoms) return fail(BAGS_ERR_ARG, "%s: NULL binoms", op);
    if (n_max < 2 || n_max > BAGS_MCMC_MAX_BINOMS) return fail(BAGS_ERR_ARG, "%s: n_max %d not in 2..%d", op, n_max, BAGS_MCMC_MAX_BINOMS);
    return BAGS_OK;
}

int bags_compute_relocation(const float* opacity_old, const float* scale_old, const int32_t* N, const float* binoms, int32_t n_max, int32_t P,
                            float* opacity_new, float* scale_new, void* stream)
{
    if (const int rc = check_binoms("compute_relocation", binoms, n_max)) return rc;
    if (P < 0) return fail(BAGS_ERR_ARG, "compute_relocation: P < 0 (got %d)", P);
    if (P == 0) return BAGS_OK;
    if (!opacity_old || !scale_old || !N) return fail(BAGS_ERR_ARG, "compute_relocation: NULL opacity_old / scale_old / N");
    if (!opacity_new || !scale_new) return fail(BAGS_ERR_ARG, "compute_relocation: NULL opacity_new / scale_new");
    HIP_TRY(launch_compute_relocation(opacity_old, scale_old, N, binoms, n_max, P, opacity_new, scale_new, (hipStream_t)stream));
    return BAGS_OK;
}

size_t bags_mcmc_workspace_size(int32_t P) { return mcmc_workspace_bytes(P); }

// what relocate and add_new share; outputs: add_new's (P + n_sampled)-row arrays are checked too
static int check_mcmc(const char* op, const BagsMcmcGroup* groups, int32_t n_groups, int32_t P, const int32_t* sampled, int32_t n_sampled,
                      const float* binoms, int32_t n_max, double min_opacity, const void* workspace, size_t workspace_bytes, bool outputs)
{
    if (const int rc = check_binoms(op, binoms, n_max)) return rc;
    if (P < 0) return fail(BAGS_ERR_ARG, "%s: P < 0 (got %d)", op, P);
    if (n_sampled < 0) return fail(BAGS_ERR_ARG, "%s: n_sampled < 0 (got %d)", op, n_sampled);
    if (!(min_opacity > 0.0 && min_opacity < 1.0)) return fail(BAGS_ERR_ARG, "%s: min_opacity %g not in (0, 1)", op, min_opacity);
    if (const int rc = check_group_count(op, groups, n_groups)) return rc;
    if (outputs && (int64_t)P + n_sampled > 0x7FFFFFFFll) return fail(BAGS_ERR_SIZE, "%s: the new set would hold %lld rows (> 2^31 - 1)", op, (long long)P + n_sampled);
    const bool work = P > 0 && n_sampled > 0;
    int n_opacity = 0, n_scaling = 0;
    for (int k = 0; k < n_groups; ++k) {
        const BagsMcmcGroup& g = groups[k];
        if (const int rc = check_group_shape(op, k, g.width, g.role)) return rc;
        n_opacity += g.role == BAGS_ROLE_OPACITY; n_scaling += g.role == BAGS_ROLE_SCALING;
        if (!work) continue;
        if (!g.param) return fail(BAGS_ERR_ARG, "%s: group %d: NULL param", op, k);
        if ((g.exp_avg != nullptr) != (g.exp_avg_sq != nullptr)) return fail(BAGS_ERR_ARG, "%s: group %d: exp_avg and exp_avg_sq are given together or not at all", op, k);
        if (outputs) {
            if (!g.param_out) return fail(BAGS_ERR_ARG, "%s: group %d: NULL param_out", op, k);
            if ((g.exp_avg != nullptr) != (g.exp_avg_out != nullptr) || (g.exp_avg != nullptr) != (g.exp_avg_sq_out != nullptr))
                return fail(BAGS_ERR_ARG, "%s: group %d: exp_avg_out and exp_avg_sq_out are given exactly when the moments are", op, k);
            if (const int rc = check_group_aligned(op, k, g.param_out, g.exp_avg_out, g.exp_avg_sq_out)) return rc;
        }
    }
    if (n_opacity != 1 || n_scaling != 1) return fail(BAGS_ERR_ARG, "%s: role opacity and scaling must each be given once (got %d, %d)", op, n_opacity, n_scaling);
    if (!work) return BAGS_OK;
    if (!sampled) return fail(BAGS_ERR_ARG, "%s: NULL sampled", op);
    if (!workspace) return fail(BAGS_ERR_ARG, "%s: NULL workspace", op);
    if (workspace_bytes < mcmc_workspace_bytes(P)) return fail(BAGS_ERR_SIZE, "%s: workspace %zu bytes < %zu", op, workspace_bytes, mcmc_workspace_bytes(P));
    return BAGS_OK;
}

int bags_mcmc_relocate(const BagsMcmcGroup* groups, int32_t n_groups, int32_t P, const int32_t* dead, const int32_t* sampled, int32_t n_sampled,
                       const float* binoms, int32_t n_max, double min_opacity, void* workspace, size_t workspace_bytes, void* stream)
{
    if (const int rc = check_mcmc("mcmc_relocate", groups, n_groups, P, sampled, n_sampled, binoms, n_max, min_opacity, workspace, workspace_bytes, false)) return rc;
    if (P == 0 || n_sampled == 0) return BAGS_OK;
    if (!dead) return fail(BAGS_ERR_ARG, "mcmc_relocate: NULL dead");
    HIP_TRY(launch_mcmc_relocate(groups, n_groups, P, dead, sampled, n_sampled, binoms, n_max, min_opacity, workspace, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_mcmc_add_new(const BagsMcmcGroup* groups, int32_t n_groups, int32_t P, const int32_t* sampled, int32_t n_sampled, const float* binoms,
                      int32_t n_max, double min_opacity, void* workspace, size_t workspace_bytes, float* accum_out, float* denom_out,
                      float* radii_out, void* stream)
{
    if (const int rc = check_mcmc("mcmc_add_new", groups, n_groups, P, sampled, n_sampled, binoms, n_max, min_opacity, workspace, workspace_bytes, true)) return rc;
    if (P == 0 || n_sampled == 0) return BAGS_OK;
    if (const int rc = check_stats_out("mcmc_add_new", accum_out, denom_out, radii_out)) return rc;
    HIP_TRY(launch_mcmc_add_new(groups, n_groups, P, sampled, n_sampled, binoms, n_max, min_opacity, workspace, accum_out, denom_out, radii_out,
                                (hipStream_t)stream));
    return BAGS_OK;
}

int bags_mcmc_noise(float* xyz, const float* opacity, const float* scaling, const float* rotation, int32_t P, const float* noise, uint64_t seed,
                    double scale, double k, double x0, double scaling_modifier, void* stream)
{
    if (P < 0) return fail(BAGS_ERR_ARG, "mcmc_noise: P < 0 (got %d)", P);
    if (!(scale == scale) || !(k == k) || !(x0 == x0) || !(scaling_modifier == scaling_modifier))
        return fail(BAGS_ERR_ARG, "mcmc_noise: scale / k / x0 / scaling_modifier is NaN");
    if (P == 0) return BAGS_OK;
    if (!xyz || !opacity || !scaling || !rotation) return fail(BAGS_ERR_ARG, "mcmc_noise: NULL xyz / opacity / scaling / rotation");
    HIP_TRY(launch_mcmc_noise(xyz, opacity, scaling, rotation, P, noise, seed, scale, k, x0, scaling_modifier, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- antialias.hip: one row of pose sums per workgroup
static size_t carve_antialias(void* base, int P, float** slab)
{
    Carver c(base);
    float* s = c.take<float>((size_t)antialias_blocks(P) * AA_SLAB);
    if (slab) *slab = s;
    return c.used();
}

size_t bags_antialias_workspace_size(int32_t P) { return carve_antialias(nullptr, P, nullptr) + BASE_SLACK; }

static int check_antialias(const char* op, const BagsAntialias* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->P < 0) return fail(BAGS_ERR_ARG, "%s: P < 0 (got %d)", op, a->P);
    if (a->image_width <= 0 || a->image_height <= 0) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->image_width, a->image_height);
    if (a->clamp_grad != BAGS_CLAMP_GRAD_STOCK && a->clamp_grad != BAGS_CLAMP_GRAD_EXACT)
        return fail(BAGS_ERR_ARG, "%s: clamp_grad %d is neither stock (0) nor exact (1)", op, a->clamp_grad);
    if (a->P == 0) return BAGS_OK;                 // an empty set has no rows to point to: the pointers are not looked at
    const bool pair = a->scales || a->rotations;
    if ((pair && a->cov3D_precomp) || (!(a->scales && a->rotations) && !a->cov3D_precomp))
        return fail(BAGS_ERR_ARG, "%s: provide exactly one of either scale/rotation pair or precomputed 3D covariance", op);
    if (!a->viewmatrix || !a->intrinsic) return fail(BAGS_ERR_ARG, "%s: NULL viewmatrix / intrinsic", op);
    if (!a->means3D || !a->opacities) return fail(BAGS_ERR_ARG, "%s: NULL means3D / opacities", op);
    return BAGS_OK;
}

int bags_antialias_forward(const BagsAntialias* a, float* out, void* stream)
{
    if (const int rc = check_antialias("antialias_forward", a)) return rc;
    if (a->P == 0) return BAGS_OK;
    if (!out) return fail(BAGS_ERR_ARG, "antialias_forward: NULL out");
    HIP_TRY(launch_antialias_fwd(*a, out, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_antialias_backward(const BagsAntialias* a, const float* grad_out, void* workspace, size_t workspace_bytes, float* g_opacities,
                            float* g_means3D, float* g_scales, float* g_rotations, float* g_cov3D, float* g_viewmatrix, float* g_intrinsic,
                            float* g_shift_factors, void* stream)
{
    if (const int rc = check_antialias("antialias_backward", a)) return rc;
    if (a->P == 0) return BAGS_OK;
    if (!grad_out) return fail(BAGS_ERR_ARG, "antialias_backward: NULL grad_out");
    if (a->cov3D_precomp ? (g_scales || g_rotations) : g_cov3D != nullptr)
        return fail(BAGS_ERR_ARG, "antialias_backward: a gradient is asked for the covariance source that was not given");
    float* slab = nullptr;
    if (g_viewmatrix || g_intrinsic || g_shift_factors) {
        const size_t need = bags_antialias_workspace_size(a->P);
        if (!workspace || workspace_bytes < need)
            return fail(BAGS_ERR_SIZE, "antialias_backward: the pose gradients need a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
        carve_antialias(workspace, a->P, &slab);
    }
    if (!g_opacities && !g_means3D && !g_scales && !g_rotations && !g_cov3D && !slab) return BAGS_OK;
    HIP_TRY(launch_antialias_bwd(*a, grad_out, slab, g_opacities, g_means3D, g_scales, g_rotations, g_cov3D, g_viewmatrix, g_intrinsic,
                                 g_shift_factors, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- appearance.hip: one row of 16 doubles per workgroup of the pixels kernel, view-major
static size_t carve_appearance(void* base, int n_rows, int H, int W, double** partials)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)n_rows * appearance_slots(H, W) * 16);
    if (partials) *partials = p;
    return c.used();
}

static bool appearance_image_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

size_t bags_appearance_workspace_size(int32_t n_rows, int32_t H, int32_t W)
{
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS || !appearance_image_ok(H, W)) return 0;
    return carve_appearance(nullptr, n_rows, H, W, nullptr);
}

static int check_appearance(const char* op, const BagsAppearance* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (!a->table) return fail(BAGS_ERR_ARG, "%s: null table", op);
    if (const int rc = check_pose_rows(op, a->N, a->n_rows, a->rows)) return rc;
    if (a->C != 3) return fail(BAGS_ERR_ARG, "%s: C must be 3 (got %d)", op, a->C);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!appearance_image_ok(a->H, a->W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, a->W, a->H);
    if (!(a->cx == a->cx) || !(a->cy == a->cy)) return fail(BAGS_ERR_ARG, "%s: the centre is NaN", op);
    for (int v = 0; v < a->n_rows; ++v)
        if (!a->image[v]) return fail(BAGS_ERR_ARG, "%s: null image[%d]", op, v);
    return BAGS_OK;
}

int bags_appearance_forward(const BagsAppearance* a, void* stream)
{
    if (const int rc = check_appearance("appearance_forward", a)) return rc;
    for (int v = 0; v < a->n_rows; ++v)
        if (!a->out[v]) return fail(BAGS_ERR_ARG, "appearance_forward: null out[%d]", v);
    HIP_TRY(launch_appearance_fwd(*a, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_appearance_backward(const BagsAppearance* a, const float* const g_out[BAGS_MAX_POSE_ROWS], void* workspace, size_t workspace_bytes,
                             float* const g_image[BAGS_MAX_POSE_ROWS], float* g_table, void* stream)
{
    if (const int rc = check_appearance("appearance_backward", a)) return rc;
    if (!g_out) return fail(BAGS_ERR_ARG, "appearance_backward: null g_out");
    for (int v = 0; v < a->n_rows; ++v)
        if (!g_out[v]) return fail(BAGS_ERR_ARG, "appearance_backward: null g_out[%d]", v);
    if (g_table == a->table) return fail(BAGS_ERR_ARG, "appearance_backward: g_table must not be the table");
    double* partials = nullptr;
    if (g_table) {
        const size_t need = bags_appearance_workspace_size(a->n_rows, a->H, a->W);
        if (!workspace || workspace_bytes < need)
            return fail(BAGS_ERR_ARG, "appearance_backward: g_table needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
        if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "appearance_backward: the workspace is not 16-byte aligned");
        carve_appearance(workspace, a->n_rows, a->H, a->W, &partials);
    }
    bool any_image = false;
    for (int v = 0; g_image && v < a->n_rows; ++v) any_image |= g_image[v] != nullptr;
    if (!any_image && !g_table) return BAGS_OK;
    HIP_TRY(launch_appearance_bwd(*a, g_out, partials, any_image ? g_image : nullptr, g_table, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- bilagrid.hip: the slice and its adjoint keep nothing between launches; the TV forward one row of 4 doubles per workgroup
static bool bilagrid_grid_ok(int Gx, int Gy, int L)
{
    return Gx >= 1 && Gx <= BAGS_BILAGRID_MAX_G && Gy >= 1 && Gy <= BAGS_BILAGRID_MAX_G && L >= 1 && L <= BAGS_BILAGRID_MAX_L;
}

static int check_bilagrid_grid(const char* op, int Gx, int Gy, int L)
{
    if (bilagrid_grid_ok(Gx, Gy, L)) return BAGS_OK;
    return fail(BAGS_ERR_ARG, "%s: grid (Gx, Gy, L) = (%d, %d, %d) is outside 1..%d, 1..%d, 1..%d (bilagrid_torch is the same function in PyTorch for any size)",
                op, Gx, Gy, L, BAGS_BILAGRID_MAX_G, BAGS_BILAGRID_MAX_G, BAGS_BILAGRID_MAX_L);
}

static int check_bilagrid(const char* op, const BagsBilagrid* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (!a->grids) return fail(BAGS_ERR_ARG, "%s: null grids", op);
    if (const int rc = check_pose_rows(op, a->N, a->n_rows, a->rows)) return rc;
    if (a->C != 3) return fail(BAGS_ERR_ARG, "%s: C must be 3 (got %d)", op, a->C);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!appearance_image_ok(a->H, a->W))
        return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more (bilagrid_torch is the same function in PyTorch for any size)", op, a->W, a->H);
    if (const int rc = check_bilagrid_grid(op, a->Gx, a->Gy, a->L)) return rc;
    if (a->path != BAGS_BILAGRID_PATH_AUTO && a->path != BAGS_BILAGRID_PATH_DIRECT) return fail(BAGS_ERR_ARG, "%s: path %d is not a BAGS_BILAGRID_PATH_*", op, a->path);
    for (int v = 0; v < a->n_rows; ++v)
        if (!a->image[v]) return fail(BAGS_ERR_ARG, "%s: null image[%d]", op, v);
    return BAGS_OK;
}

int bags_bilagrid_forward(const BagsBilagrid* a, void* stream)
{
    if (const int rc = check_bilagrid("bilagrid_forward", a)) return rc;
    for (int v = 0; v < a->n_rows; ++v)
        if (!a->out[v]) return fail(BAGS_ERR_ARG, "bilagrid_forward: null out[%d]", v);
    HIP_TRY(launch_bilagrid_fwd(*a, (hipStream_t)stream));
    return BAGS_OK;
}

size_t bags_bilagrid_workspace_size(int32_t, int32_t, int32_t) { return 0; }     // a vertex's sums are one workgroup's: nothing is kept

int bags_bilagrid_backward(const BagsBilagrid* a, const float* const g_out[BAGS_MAX_POSE_ROWS], void* /*workspace*/, size_t /*workspace_bytes*/,
                           float* const g_image[BAGS_MAX_POSE_ROWS], float* g_grids, void* stream)
{
    if (const int rc = check_bilagrid("bilagrid_backward", a)) return rc;
    if (!g_out) return fail(BAGS_ERR_ARG, "bilagrid_backward: null g_out");
    for (int v = 0; v < a->n_rows; ++v)
        if (!g_out[v]) return fail(BAGS_ERR_ARG, "bilagrid_backward: null g_out[%d]", v);
    if (g_grids == a->grids) return fail(BAGS_ERR_ARG, "bilagrid_backward: g_grids must not be the grids");
    bool any_image = false;
    for (int v = 0; g_image && v < a->n_rows; ++v) any_image |= g_image[v] != nullptr;
    if (!any_image && !g_grids) return BAGS_OK;
    HIP_TRY(launch_bilagrid_bwd(*a, g_out, any_image ? g_image : nullptr, g_grids, (hipStream_t)stream));
    return BAGS_OK;
}

static size_t carve_bilagrid_tv(void* base, int N, int Gx, int Gy, int L, double** partials)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)bilagrid_tv_blocks((long long)N * 12 * L * Gy * Gx) * 4);
    if (partials) *partials = p;
    return c.used();
}

size_t bags_bilagrid_tv_workspace_size(int32_t N, int32_t Gx, int32_t Gy, int32_t L)
{
    if (N < 1 || !bilagrid_grid_ok(Gx, Gy, L)) return 0;
    return carve_bilagrid_tv(nullptr, N, Gx, Gy, L, nullptr);
}

int bags_bilagrid_tv_forward(const float* grids, int32_t N, int32_t Gx, int32_t Gy, int32_t L, void* workspace, size_t workspace_bytes, float* loss,
                             void* stream)
{
    if (N < 1) return fail(BAGS_ERR_ARG, "bilagrid_tv_forward: N %d < 1", N);
    if (const int rc = check_bilagrid_grid("bilagrid_tv_forward", Gx, Gy, L)) return rc;
    if (!grids) return fail(BAGS_ERR_ARG, "bilagrid_tv_forward: null grids");
    if (!loss) return fail(BAGS_ERR_ARG, "bilagrid_tv_forward: null loss");
    const size_t need = bags_bilagrid_tv_workspace_size(N, Gx, Gy, L);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "bilagrid_tv_forward: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "bilagrid_tv_forward: the workspace is not 16-byte aligned");
    double* partials = nullptr;
    carve_bilagrid_tv(workspace, N, Gx, Gy, L, &partials);
    HIP_TRY(launch_bilagrid_tv_fwd(grids, N, Gx, Gy, L, partials, loss, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_bilagrid_tv_backward(const float* grids, int32_t N, int32_t Gx, int32_t Gy, int32_t L, const float* g_loss, float* g_grids, void* stream)
{
    if (N < 1) return fail(BAGS_ERR_ARG, "bilagrid_tv_backward: N %d < 1", N);
    if (const int rc = check_bilagrid_grid("bilagrid_tv_backward", Gx, Gy, L)) return rc;
    if (!grids) return fail(BAGS_ERR_ARG, "bilagrid_tv_backward: null grids");
    if (!g_loss) return fail(BAGS_ERR_ARG, "bilagrid_tv_backward: null g_loss");
    if (!g_grids) return fail(BAGS_ERR_ARG, "bilagrid_tv_backward: null g_grids");
    if (g_grids == grids) return fail(BAGS_ERR_ARG, "bilagrid_tv_backward: g_grids must not be the grids");
    HIP_TRY(launch_bilagrid_tv_bwd(grids, N, Gx, Gy, L, g_loss, g_grids, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- filter3d.hip: a dist per Gaussian and a maximum per workgroup between the two launches
static size_t carve_filter3d(void* base, int P, float** dist, float** partials)
{
    Carver c(base);
    float* d = c.take<float>((size_t)(P > 0 ? P : 0));
    float* p = c.take<float>((size_t)filter3d_blocks(P));
    if (dist) *dist = d;
    if (partials) *partials = p;
    return c.used();
}

size_t bags_filter3d_workspace_size(int32_t P) { return carve_filter3d(nullptr, P, nullptr, nullptr) + BASE_SLACK; }

int bags_filter3d_compute(const float* xyz, int32_t P, const float* viewmatrices, const float* intrinsics, const int32_t* sizes, int32_t N,
                          float variance, void* workspace, size_t workspace_bytes, float* out, void* stream)
{
    if (P < 0) return fail(BAGS_ERR_ARG, "filter3d_compute: P < 0 (got %d)", P);
    if (N <= 0) return fail(BAGS_ERR_ARG, "filter3d_compute: needs at least one camera (N = %d)", N);
    if (!(variance >= 0.0f)) return fail(BAGS_ERR_ARG, "filter3d_compute: variance is negative or NaN");
    if (P == 0) return BAGS_OK;
    if (!xyz || !viewmatrices || !intrinsics || !sizes || !out) return fail(BAGS_ERR_ARG, "filter3d_compute: NULL xyz / viewmatrices / intrinsics / sizes / out");
    const size_t need = bags_filter3d_workspace_size(P);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_SIZE, "filter3d_compute: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    float *dist = nullptr, *partials = nullptr;
    carve_filter3d(workspace, P, &dist, &partials);
    HIP_TRY(launch_filter3d(xyz, P, viewmatrices, intrinsics, sizes, N, variance, dist, partials, out, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- depth_prior.hip: one row of 8 doubles per workgroup of the sums kernel, view-major
static size_t carve_depth_prior(void* base, int n_rows, int H, int W, double** partials)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)n_rows * depth_prior_slots(H, W) * BAGS_DEPTH_PRIOR_STATS);
    if (partials) *partials = p;
    return c.used();
}

static bool depth_prior_image_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

size_t bags_depth_prior_workspace_size(int32_t n_rows, int32_t H, int32_t W)
{
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS || !depth_prior_image_ok(H, W)) return 0;
    return carve_depth_prior(nullptr, n_rows, H, W, nullptr);
}

static int check_depth_prior(const char* op, const BagsDepthPrior* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->mode != BAGS_DEPTH_PRIOR_PEARSON && a->mode != BAGS_DEPTH_PRIOR_L1) return fail(BAGS_ERR_ARG, "%s: unknown mode %d", op, a->mode);
    if (a->space != BAGS_DEPTH_PRIOR_DEPTH && a->space != BAGS_DEPTH_PRIOR_INVERSE) return fail(BAGS_ERR_ARG, "%s: unknown space %d", op, a->space);
    if (a->table) {
        if (a->mode == BAGS_DEPTH_PRIOR_PEARSON) return fail(BAGS_ERR_ARG, "%s: a table with the pearson mode (it has no parameters)", op);
        if (const int rc = check_pose_rows(op, a->N, a->n_rows, a->rows)) return rc;
    } else if (a->n_rows < 1 || a->n_rows > BAGS_MAX_POSE_ROWS)
        return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, a->n_rows, BAGS_MAX_POSE_ROWS);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!depth_prior_image_ok(a->H, a->W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, a->W, a->H);
    if (!(a->min_weight == a->min_weight)) return fail(BAGS_ERR_ARG, "%s: min_weight is NaN", op);
    for (int v = 0; v < a->n_rows; ++v) {
        if (!a->depth[v]) return fail(BAGS_ERR_ARG, "%s: null depth[%d]", op, v);
        if (!a->weights[v]) return fail(BAGS_ERR_ARG, "%s: null weights[%d]", op, v);
        if (!a->prior[v]) return fail(BAGS_ERR_ARG, "%s: null prior[%d]", op, v);
    }
    return BAGS_OK;
}

int bags_depth_prior_forward(const BagsDepthPrior* a, void* workspace, size_t workspace_bytes, float* loss, float* count, double* stats,
                             void* stream)
{
    if (const int rc = check_depth_prior("depth_prior_forward", a)) return rc;
    if (!loss || !count || !stats) return fail(BAGS_ERR_ARG, "depth_prior_forward: null loss / count / stats");
    const size_t need = bags_depth_prior_workspace_size(a->n_rows, a->H, a->W);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "depth_prior_forward: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "depth_prior_forward: the workspace is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "depth_prior_forward: stats is not 8-byte aligned");
    double* partials = nullptr;
    carve_depth_prior(workspace, a->n_rows, a->H, a->W, &partials);
    HIP_TRY(launch_depth_prior_fwd(*a, partials, loss, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_depth_prior_backward(const BagsDepthPrior* a, const double* stats, const float* g_loss, float* const g_depth[BAGS_MAX_POSE_ROWS],
                              float* const g_weights[BAGS_MAX_POSE_ROWS], float* g_table, void* stream)
{
    if (const int rc = check_depth_prior("depth_prior_backward", a)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "depth_prior_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "depth_prior_backward: stats is not 8-byte aligned");
    if (!g_loss) return fail(BAGS_ERR_ARG, "depth_prior_backward: null g_loss");
    if (g_table && !a->table) return fail(BAGS_ERR_ARG, "depth_prior_backward: g_table is asked for but no table was given");
    if (g_table && g_table == a->table) return fail(BAGS_ERR_ARG, "depth_prior_backward: g_table must not be the table");
    bool any_map = false;
    for (int v = 0; v < a->n_rows; ++v) any_map |= (g_depth && g_depth[v]) || (g_weights && g_weights[v]);
    if (!any_map && !g_table) return BAGS_OK;
    HIP_TRY(launch_depth_prior_bwd(*a, stats, g_loss, g_depth, g_weights, g_table, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- normal_prior.hip: one row of 2 doubles per tile, view-major
static size_t carve_normal_prior(void* base, int n_rows, int H, int W, double** partials)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)n_rows * (size_t)normal_prior_tiles(H, W) * BAGS_NORMAL_PRIOR_STATS);
    if (partials) *partials = p;
    return c.used();
}

// the rows of tiles are grid dimension y
static bool normal_prior_image_ok(int H, int W)
{
    return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31) && (H + BAGS_NORMAL_PRIOR_TILE_H - 1) / BAGS_NORMAL_PRIOR_TILE_H <= 65535;
}

size_t bags_normal_prior_workspace_size(int32_t n_rows, int32_t H, int32_t W)
{
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS || !normal_prior_image_ok(H, W)) return 0;
    return carve_normal_prior(nullptr, n_rows, H, W, nullptr);
}

static int check_normal_geometry(const char* op, int H, int W, float min_weight, float max_jump)
{
    if (H < 1 || W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, W, H);
    if ((long long)H * W >= (1ll << 31)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, W, H);
    if (!normal_prior_image_ok(H, W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has more than %d rows", op, W, H, 65535 * BAGS_NORMAL_PRIOR_TILE_H);
    if (!(min_weight > 0.0f) || std::isinf(min_weight)) return fail(BAGS_ERR_ARG, "%s: min_weight must be a positive number", op);
    if (!(max_jump >= 0.0f)) return fail(BAGS_ERR_ARG, "%s: max_jump must be a non-negative number or inf", op);
    return BAGS_OK;
}

static int check_pinhole(const char* op, int v, const double* p)
{
    for (int j = 0; j < 4; ++j)
        if (!std::isfinite(p[j])) return fail(BAGS_ERR_ARG, "%s: pinhole[%d] is not finite", op, v);
    if (p[0] == 0.0 || p[1] == 0.0) return fail(BAGS_ERR_ARG, "%s: pinhole[%d] has a zero focal length", op, v);
    return BAGS_OK;
}

static int check_normal_prior(const char* op, const BagsNormalPrior* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->mode != BAGS_NORMAL_PRIOR_COS && a->mode != BAGS_NORMAL_PRIOR_L1) return fail(BAGS_ERR_ARG, "%s: unknown mode %d", op, a->mode);
    if (a->n_rows < 1 || a->n_rows > BAGS_MAX_POSE_ROWS) return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, a->n_rows, BAGS_MAX_POSE_ROWS);
    if (const int rc = check_normal_geometry(op, a->H, a->W, a->min_weight, a->max_jump)) return rc;
    for (int v = 0; v < a->n_rows; ++v) {
        if (const int rc = check_pinhole(op, v, a->pinhole[v])) return rc;
        if (!a->depth[v]) return fail(BAGS_ERR_ARG, "%s: null depth[%d]", op, v);
        if (!a->weights[v]) return fail(BAGS_ERR_ARG, "%s: null weights[%d]", op, v);
        if (!a->prior[v]) return fail(BAGS_ERR_ARG, "%s: null prior[%d]", op, v);
    }
    return BAGS_OK;
}

int bags_normal_prior_forward(const BagsNormalPrior* a, void* workspace, size_t workspace_bytes, float* loss, float* count, double* stats,
                              void* stream)
{
    if (const int rc = check_normal_prior("normal_prior_forward", a)) return rc;
    if (!loss || !count || !stats) return fail(BAGS_ERR_ARG, "normal_prior_forward: null loss / count / stats");
    const size_t need = bags_normal_prior_workspace_size(a->n_rows, a->H, a->W);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "normal_prior_forward: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "normal_prior_forward: the workspace is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "normal_prior_forward: stats is not 8-byte aligned");
    double* partials = nullptr;
    carve_normal_prior(workspace, a->n_rows, a->H, a->W, &partials);
    HIP_TRY(launch_normal_prior_fwd(*a, partials, loss, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_normal_prior_backward(const BagsNormalPrior* a, const double* stats, const float* g_loss, float* const g_depth[BAGS_MAX_POSE_ROWS],
                               float* const g_weights[BAGS_MAX_POSE_ROWS], void* stream)
{
    if (const int rc = check_normal_prior("normal_prior_backward", a)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "normal_prior_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "normal_prior_backward: stats is not 8-byte aligned");
    if (!g_loss) return fail(BAGS_ERR_ARG, "normal_prior_backward: null g_loss");
    bool any_map = false;
    for (int v = 0; v < a->n_rows; ++v) any_map |= (g_depth && g_depth[v]) || (g_weights && g_weights[v]);
    if (!any_map) return BAGS_OK;
    HIP_TRY(launch_normal_prior_bwd(*a, stats, g_loss, g_depth, g_weights, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_depth_to_normal(const float* depth, const float* weights, int32_t H, int32_t W, const double pinhole[4], float min_weight,
                         float max_jump, float* normal, uint8_t* valid, void* stream)
{
    if (const int rc = check_normal_geometry("depth_to_normal", H, W, min_weight, max_jump)) return rc;
    if (!pinhole) return fail(BAGS_ERR_ARG, "depth_to_normal: null pinhole");
    if (const int rc = check_pinhole("depth_to_normal", 0, pinhole)) return rc;
    if (!depth || !weights) return fail(BAGS_ERR_ARG, "depth_to_normal: null depth / weights");
    if (!normal || !valid) return fail(BAGS_ERR_ARG, "depth_to_normal: null normal / valid");
    HIP_TRY(launch_depth_to_normal(depth, weights, H, W, pinhole, min_weight, max_jump, normal, valid, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- correspondence.hip: per pair and chunk one row of 2 doubles forward, 12 doubles backward; one size serves both
static size_t carve_correspondence(void* base, int n_rows, int H, int W, double** partials)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)n_rows * (size_t)correspondence_chunks(H, W) * BAGS_CORRESPONDENCE_SUMS);
    if (partials) *partials = p;
    return c.used();
}

static bool correspondence_image_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W < (1ll << 31); }

size_t bags_correspondence_workspace_size(int32_t n_rows, int32_t H, int32_t W)
{
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS || !correspondence_image_ok(H, W)) return 0;
    return carve_correspondence(nullptr, n_rows, H, W, nullptr);
}

static int check_correspondence(const char* op, const BagsCorrespondence* a, bool matches)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->n_rows < 1 || a->n_rows > BAGS_MAX_POSE_ROWS) return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, a->n_rows, BAGS_MAX_POSE_ROWS);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!correspondence_image_ok(a->H, a->W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, a->W, a->H);
    if (!(a->min_weight > 0.0f) || std::isinf(a->min_weight)) return fail(BAGS_ERR_ARG, "%s: min_weight must be a positive number", op);
    if (!(a->min_depth > 0.0) || std::isinf(a->min_depth)) return fail(BAGS_ERR_ARG, "%s: min_depth must be a positive number", op);
    if (!(a->delta > 0.0)) return fail(BAGS_ERR_ARG, "%s: delta must be a positive number or inf", op);
    for (int k = 0; k < a->n_rows; ++k) {
        if (const int rc = check_pinhole(op, k, a->pinhole_src[k])) return rc;
        if (const int rc = check_pinhole(op, k, a->pinhole_dst[k])) return rc;
        if (!a->depth[k]) return fail(BAGS_ERR_ARG, "%s: null depth[%d]", op, k);
        if (!a->weights[k]) return fail(BAGS_ERR_ARG, "%s: null weights[%d]", op, k);
        if (matches && !a->match[k]) return fail(BAGS_ERR_ARG, "%s: null match[%d]", op, k);
        if (!a->view_src[k] || !a->view_dst[k]) return fail(BAGS_ERR_ARG, "%s: null view_src[%d] / view_dst[%d]", op, k, k);
    }
    return BAGS_OK;
}

static int check_correspondence_workspace(const char* op, const BagsCorrespondence* a, void* workspace, size_t workspace_bytes)
{
    const size_t need = bags_correspondence_workspace_size(a->n_rows, a->H, a->W);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "%s: needs a workspace of %zu bytes (got %zu)", op, need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "%s: the workspace is not 16-byte aligned", op);
    return BAGS_OK;
}

int bags_correspondence_forward(const BagsCorrespondence* a, void* workspace, size_t workspace_bytes, float* loss, float* count, double* stats,
                                void* stream)
{
    if (const int rc = check_correspondence("correspondence_forward", a, true)) return rc;
    if (!loss || !count || !stats) return fail(BAGS_ERR_ARG, "correspondence_forward: null loss / count / stats");
    if (const int rc = check_correspondence_workspace("correspondence_forward", a, workspace, workspace_bytes)) return rc;
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "correspondence_forward: stats is not 8-byte aligned");
    double* partials = nullptr;
    carve_correspondence(workspace, a->n_rows, a->H, a->W, &partials);
    HIP_TRY(launch_correspondence_fwd(*a, partials, loss, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_correspondence_backward(const BagsCorrespondence* a, const double* stats, const float* g_loss, void* workspace, size_t workspace_bytes,
                                 float* const g_depth[BAGS_MAX_POSE_ROWS], float* const g_weights[BAGS_MAX_POSE_ROWS],
                                 float* const g_view_src[BAGS_MAX_POSE_ROWS], float* const g_view_dst[BAGS_MAX_POSE_ROWS], void* stream)
{
    if (const int rc = check_correspondence("correspondence_backward", a, true)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "correspondence_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "correspondence_backward: stats is not 8-byte aligned");
    if (!g_loss) return fail(BAGS_ERR_ARG, "correspondence_backward: null g_loss");
    bool any_map = false, any_view = false;
    for (int k = 0; k < a->n_rows; ++k) {
        any_map |= (g_depth && g_depth[k]) || (g_weights && g_weights[k]);
        any_view |= (g_view_src && g_view_src[k]) || (g_view_dst && g_view_dst[k]);
    }
    if (!any_map && !any_view) return BAGS_OK;
    double* sums = nullptr;
    if (any_view) {
        if (const int rc = check_correspondence_workspace("correspondence_backward", a, workspace, workspace_bytes)) return rc;
        carve_correspondence(workspace, a->n_rows, a->H, a->W, &sums);
    }
    HIP_TRY(launch_correspondence_bwd(*a, stats, g_loss, sums, g_depth, g_weights, g_view_src, g_view_dst, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_reproject_pixels(const BagsCorrespondence* a, int32_t H_dst, int32_t W_dst, float* proj, uint8_t* valid, void* stream)
{
    if (const int rc = check_correspondence("reproject_pixels", a, false)) return rc;
    if (a->n_rows != 1) return fail(BAGS_ERR_ARG, "reproject_pixels: one pair per call (n_rows = %d)", a->n_rows);
    if (H_dst < 1 || W_dst < 1) return fail(BAGS_ERR_ARG, "reproject_pixels: empty target image %dx%d", W_dst, H_dst);
    if (!proj || !valid) return fail(BAGS_ERR_ARG, "reproject_pixels: null proj / valid");
    HIP_TRY(launch_reproject_pixels(*a, H_dst, W_dst, proj, valid, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- warp.hip: the rows of correspondence.hip, per pair and chunk of the SOURCE image, carved by carve_correspondence
size_t bags_warp_workspace_size(int32_t n_rows, int32_t H, int32_t W)
{
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS || !correspondence_image_ok(H, W)) return 0;
    return carve_correspondence(nullptr, n_rows, H, W, nullptr);
}

static int check_warp(const char* op, const BagsWarp* a, bool colors)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->n_rows < 1 || a->n_rows > BAGS_MAX_POSE_ROWS) return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, a->n_rows, BAGS_MAX_POSE_ROWS);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!correspondence_image_ok(a->H, a->W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, a->W, a->H);
    if (a->H_dst < 1 || a->W_dst < 1) return fail(BAGS_ERR_ARG, "%s: empty target image %dx%d", op, a->W_dst, a->H_dst);
    if (!correspondence_image_ok(a->H_dst, a->W_dst))
        return fail(BAGS_ERR_ARG, "%s: target image %dx%d has 2^31 pixels or more", op, a->W_dst, a->H_dst);
    if (a->C != 1 && a->C != 3) return fail(BAGS_ERR_ARG, "%s: C = %d channels, must be 1 or 3", op, a->C);
    if (!(a->min_weight > 0.0f) || std::isinf(a->min_weight)) return fail(BAGS_ERR_ARG, "%s: min_weight must be a positive number", op);
    if (!(a->min_depth > 0.0) || std::isinf(a->min_depth)) return fail(BAGS_ERR_ARG, "%s: min_depth must be a positive number", op);
    if (!(a->eps > 0.0) || std::isinf(a->eps)) return fail(BAGS_ERR_ARG, "%s: eps must be a positive number", op);
    if (!(a->occlusion > 0.0) || std::isinf(a->occlusion)) return fail(BAGS_ERR_ARG, "%s: occlusion must be a positive number", op);
    for (int k = 0; k < a->n_rows; ++k) {
        if (const int rc = check_pinhole(op, k, a->pinhole_src[k])) return rc;
        if (const int rc = check_pinhole(op, k, a->pinhole_dst[k])) return rc;
        if (!a->depth[k]) return fail(BAGS_ERR_ARG, "%s: null depth[%d]", op, k);
        if (!a->weights[k]) return fail(BAGS_ERR_ARG, "%s: null weights[%d]", op, k);
        if (!a->view_src[k] || !a->view_dst[k]) return fail(BAGS_ERR_ARG, "%s: null view_src[%d] / view_dst[%d]", op, k, k);
        if (colors && !a->color_src[k]) return fail(BAGS_ERR_ARG, "%s: null color_src[%d]", op, k);
        if (!a->image_dst[k]) return fail(BAGS_ERR_ARG, "%s: null image_dst[%d]", op, k);
        if (!a->depth_dst[k] != !a->weights_dst[k])
            return fail(BAGS_ERR_ARG, "%s: depth_dst[%d] and weights_dst[%d] must be given together or not at all", op, k, k);
    }
    return BAGS_OK;
}

static int check_warp_workspace(const char* op, const BagsWarp* a, void* workspace, size_t workspace_bytes)
{
    const size_t need = bags_warp_workspace_size(a->n_rows, a->H, a->W);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "%s: needs a workspace of %zu bytes (got %zu)", op, need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "%s: the workspace is not 16-byte aligned", op);
    return BAGS_OK;
}

int bags_warp_forward(const BagsWarp* a, void* workspace, size_t workspace_bytes, float* loss, float* count, double* stats, void* stream)
{
    if (const int rc = check_warp("warp_forward", a, true)) return rc;
    if (!loss || !count || !stats) return fail(BAGS_ERR_ARG, "warp_forward: null loss / count / stats");
    if (const int rc = check_warp_workspace("warp_forward", a, workspace, workspace_bytes)) return rc;
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "warp_forward: stats is not 8-byte aligned");
    double* partials = nullptr;
    carve_correspondence(workspace, a->n_rows, a->H, a->W, &partials);
    HIP_TRY(launch_warp_fwd(*a, partials, loss, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_warp_backward(const BagsWarp* a, const double* stats, const float* g_loss, void* workspace, size_t workspace_bytes,
                       float* const g_depth[BAGS_MAX_POSE_ROWS], float* const g_weights[BAGS_MAX_POSE_ROWS],
                       float* const g_view_src[BAGS_MAX_POSE_ROWS], float* const g_view_dst[BAGS_MAX_POSE_ROWS], void* stream)
{
    if (const int rc = check_warp("warp_backward", a, true)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "warp_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "warp_backward: stats is not 8-byte aligned");
    if (!g_loss) return fail(BAGS_ERR_ARG, "warp_backward: null g_loss");
    bool any_map = false, any_view = false;
    for (int k = 0; k < a->n_rows; ++k) {
        any_map |= (g_depth && g_depth[k]) || (g_weights && g_weights[k]);
        any_view |= (g_view_src && g_view_src[k]) || (g_view_dst && g_view_dst[k]);
    }
    if (!any_map && !any_view) return BAGS_OK;
    double* sums = nullptr;
    if (any_view) {
        if (const int rc = check_warp_workspace("warp_backward", a, workspace, workspace_bytes)) return rc;
        carve_correspondence(workspace, a->n_rows, a->H, a->W, &sums);
    }
    HIP_TRY(launch_warp_bwd(*a, stats, g_loss, sums, g_depth, g_weights, g_view_src, g_view_dst, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_warp_image(const BagsWarp* a, float* out, uint8_t* valid, void* stream)
{
    if (const int rc = check_warp("warp_image", a, false)) return rc;
    if (a->n_rows != 1) return fail(BAGS_ERR_ARG, "warp_image: one pair per call (n_rows = %d)", a->n_rows);
    if (!out || !valid) return fail(BAGS_ERR_ARG, "warp_image: null out / valid");
    HIP_TRY(launch_warp_image(*a, out, valid, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- gaussian_normals.hip: one row of 9 V view-matrix sums per workgroup
static size_t carve_gaussian_normals(void* base, int P, int V, float** slab)
{
    Carver c(base);
    float* s = c.take<float>((size_t)gaussian_normals_blocks(P) * GN_SLAB_PER_VIEW * V);
    if (slab) *slab = s;
    return c.used();
}

size_t bags_gaussian_normals_workspace_size(int32_t P, int32_t V)
{
    if (P < 0 || V < 1 || V > BAGS_MAX_SH_VIEWS) return 0;
    return carve_gaussian_normals(nullptr, P, V, nullptr) + BASE_SLACK;
}

static int check_gaussian_normals(const char* op, const BagsGaussianNormals* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->P < 0) return fail(BAGS_ERR_ARG, "%s: P < 0 (got %d)", op, a->P);
    if (a->V < 1 || a->V > BAGS_MAX_SH_VIEWS)
        return fail(BAGS_ERR_ARG, "%s: V %d not in 1..%d (more views: one call per chunk)", op, a->V, BAGS_MAX_SH_VIEWS);
    if (a->P == 0) return BAGS_OK;                 // an empty set has no rows to point to: the pointers are not looked at
    if (!a->rotations || !a->scales || !a->means3D) return fail(BAGS_ERR_ARG, "%s: NULL rotations / scales / means3D", op);
    for (int v = 0; v < a->V; ++v)
        if (!a->viewmatrix[v]) return fail(BAGS_ERR_ARG, "%s: viewmatrix[%d] is NULL (V = %d)", op, v, a->V);
    return BAGS_OK;
}

int bags_gaussian_normals_forward(const BagsGaussianNormals* a, float* const out[], void* stream)
{
    if (const int rc = check_gaussian_normals("gaussian_normals_forward", a)) return rc;
    if (a->P == 0) return BAGS_OK;
    if (!out) return fail(BAGS_ERR_ARG, "gaussian_normals_forward: null out table");
    for (int v = 0; v < a->V; ++v)
        if (!out[v]) return fail(BAGS_ERR_ARG, "gaussian_normals_forward: out[%d] is NULL (V = %d)", v, a->V);
    HIP_TRY(launch_gaussian_normals_fwd(*a, out, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_gaussian_normals_backward(const BagsGaussianNormals* a, const float* const grad_out[], void* workspace, size_t workspace_bytes,
                                   float* g_rotations, float* const g_viewmatrix[], void* stream)
{
    if (const int rc = check_gaussian_normals("gaussian_normals_backward", a)) return rc;
    if (a->P == 0) return BAGS_OK;
    if (!grad_out) return fail(BAGS_ERR_ARG, "gaussian_normals_backward: null grad_out table (its entries may be NULL, the table not)");
    bool any_view = false;
    for (int v = 0; v < a->V; ++v) any_view |= g_viewmatrix && g_viewmatrix[v];
    float* slab = nullptr;
    if (any_view) {
        const size_t need = bags_gaussian_normals_workspace_size(a->P, a->V);
        if (!workspace || workspace_bytes < need)
            return fail(BAGS_ERR_SIZE, "gaussian_normals_backward: the view-matrix gradients need a workspace of %zu bytes (got %zu)", need,
                        workspace ? workspace_bytes : (size_t)0);
        carve_gaussian_normals(workspace, a->P, a->V, &slab);
    }
    if (!g_rotations && !slab) return BAGS_OK;
    HIP_TRY(launch_gaussian_normals_bwd(*a, grad_out, slab, g_rotations, g_viewmatrix, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- normal_map.hip: one row of 2 doubles per workgroup of the sums kernel, view-major; the slots are depth_prior.hip's
static size_t carve_normal_map(void* base, int n_rows, int H, int W, double** partials)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)n_rows * depth_prior_slots(H, W) * BAGS_NORMAL_MAP_STATS);
    if (partials) *partials = p;
    return c.used();
}

size_t bags_normal_map_workspace_size(int32_t n_rows, int32_t H, int32_t W)
{
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS || !depth_prior_image_ok(H, W)) return 0;
    return carve_normal_map(nullptr, n_rows, H, W, nullptr);
}

static int check_normal_map(const char* op, const BagsNormalMap* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->mode != BAGS_NORMAL_PRIOR_COS && a->mode != BAGS_NORMAL_PRIOR_L1) return fail(BAGS_ERR_ARG, "%s: unknown mode %d", op, a->mode);
    if (a->n_rows < 1 || a->n_rows > BAGS_MAX_POSE_ROWS) return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, a->n_rows, BAGS_MAX_POSE_ROWS);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!depth_prior_image_ok(a->H, a->W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, a->W, a->H);
    if (!(a->min_weight == a->min_weight)) return fail(BAGS_ERR_ARG, "%s: min_weight is NaN", op);
    if (!(a->min_norm >= 0.0f)) return fail(BAGS_ERR_ARG, "%s: min_norm must be a non-negative number", op);
    for (int v = 0; v < a->n_rows; ++v) {
        if (!a->normal[v]) return fail(BAGS_ERR_ARG, "%s: null normal[%d]", op, v);
        if (!a->weights[v]) return fail(BAGS_ERR_ARG, "%s: null weights[%d]", op, v);
        if (!a->prior[v]) return fail(BAGS_ERR_ARG, "%s: null prior[%d]", op, v);
    }
    return BAGS_OK;
}

int bags_normal_map_forward(const BagsNormalMap* a, void* workspace, size_t workspace_bytes, float* loss, float* count, double* stats,
                            void* stream)
{
    if (const int rc = check_normal_map("normal_map_forward", a)) return rc;
    if (!loss || !count || !stats) return fail(BAGS_ERR_ARG, "normal_map_forward: null loss / count / stats");
    const size_t need = bags_normal_map_workspace_size(a->n_rows, a->H, a->W);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "normal_map_forward: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "normal_map_forward: the workspace is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "normal_map_forward: stats is not 8-byte aligned");
    double* partials = nullptr;
    carve_normal_map(workspace, a->n_rows, a->H, a->W, &partials);
    HIP_TRY(launch_normal_map_fwd(*a, partials, loss, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_normal_map_backward(const BagsNormalMap* a, const double* stats, const float* g_loss, float* const g_normal[BAGS_MAX_POSE_ROWS],
                             void* stream)
{
    if (const int rc = check_normal_map("normal_map_backward", a)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "normal_map_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "normal_map_backward: stats is not 8-byte aligned");
    if (!g_loss) return fail(BAGS_ERR_ARG, "normal_map_backward: null g_loss");
    bool any_map = false;
    for (int v = 0; v < a->n_rows; ++v) any_map |= g_normal && g_normal[v];
    if (!any_map) return BAGS_OK;
    HIP_TRY(launch_normal_map_bwd(*a, stats, g_loss, g_normal, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- smooth.hip: one row of 6 doubles per tile of the sums kernel, then one row of 2 doubles per workgroup of the mean kernel,
// both view-major
static size_t carve_smooth(void* base, int n_rows, int H, int W, double** partials, double** mean_rows)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)n_rows * (size_t)smooth_tiles(H, W) * BAGS_SMOOTH_PARTIALS);
    double* m = c.take<double>((size_t)n_rows * (size_t)smooth_mean_slots(H, W) * 2);
    if (partials) *partials = p;
    if (mean_rows) *mean_rows = m;
    return c.used();
}

size_t bags_smooth_workspace_size(int32_t n_rows, int32_t H, int32_t W)
{
    if (n_rows < 1 || n_rows > BAGS_MAX_POSE_ROWS || !depth_prior_image_ok(H, W)) return 0;
    return carve_smooth(nullptr, n_rows, H, W, nullptr, nullptr);
}

static int check_smooth(const char* op, const BagsSmooth* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->kind != BAGS_SMOOTH_DEPTH && a->kind != BAGS_SMOOTH_NORMAL) return fail(BAGS_ERR_ARG, "%s: unknown kind %d", op, a->kind);
    if (a->kind == BAGS_SMOOTH_DEPTH && a->space != BAGS_DEPTH_PRIOR_DEPTH && a->space != BAGS_DEPTH_PRIOR_INVERSE)
        return fail(BAGS_ERR_ARG, "%s: unknown space %d", op, a->space);
    if (a->order != 1 && a->order != 2) return fail(BAGS_ERR_ARG, "%s: order must be 1 or 2 (got %d)", op, a->order);
    if (a->penalty != BAGS_SMOOTH_L1 && a->penalty != BAGS_SMOOTH_L2) return fail(BAGS_ERR_ARG, "%s: unknown penalty %d", op, a->penalty);
    if (a->normalize != 0 && a->normalize != 1) return fail(BAGS_ERR_ARG, "%s: normalize must be 0 or 1 (got %d)", op, a->normalize);
    if (a->kind == BAGS_SMOOTH_NORMAL && a->normalize) return fail(BAGS_ERR_ARG, "%s: normalize with the normal kind (unit normals have no scale)", op);
    if (a->n_rows < 1 || a->n_rows > BAGS_MAX_POSE_ROWS) return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, a->n_rows, BAGS_MAX_POSE_ROWS);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!depth_prior_image_ok(a->H, a->W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, a->W, a->H);
    if (a->guide_channels != 0 && a->guide_channels != 1 && a->guide_channels != 3)
        return fail(BAGS_ERR_ARG, "%s: guide_channels must be 0, 1 or 3 (got %d)", op, a->guide_channels);
    if (!(a->min_weight == a->min_weight)) return fail(BAGS_ERR_ARG, "%s: min_weight is NaN", op);
    if (a->kind == BAGS_SMOOTH_NORMAL && !(a->min_norm >= 0.0f)) return fail(BAGS_ERR_ARG, "%s: min_norm must be a non-negative number", op);
    if (!(a->eps >= 0.0 && a->eps < (double)INFINITY)) return fail(BAGS_ERR_ARG, "%s: eps must be a non-negative number", op);
    if (a->penalty == BAGS_SMOOTH_L2 && a->eps != 0.0) return fail(BAGS_ERR_ARG, "%s: eps must be 0 with the l2 penalty", op);
    if (!(a->gamma >= 0.0 && a->gamma < (double)INFINITY)) return fail(BAGS_ERR_ARG, "%s: gamma must be a non-negative number", op);
    for (int v = 0; v < a->n_rows; ++v) {
        if (!a->field[v]) return fail(BAGS_ERR_ARG, "%s: null field[%d]", op, v);
        if (!a->weights[v]) return fail(BAGS_ERR_ARG, "%s: null weights[%d]", op, v);
        if (a->guide_channels && !a->guide[v]) return fail(BAGS_ERR_ARG, "%s: null guide[%d]", op, v);
    }
    return BAGS_OK;
}

int bags_smooth_forward(const BagsSmooth* a, void* workspace, size_t workspace_bytes, float* loss, float* count, double* stats, void* stream)
{
    if (const int rc = check_smooth("smooth_forward", a)) return rc;
    if (!loss || !count || !stats) return fail(BAGS_ERR_ARG, "smooth_forward: null loss / count / stats");
    const size_t need = bags_smooth_workspace_size(a->n_rows, a->H, a->W);
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "smooth_forward: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "smooth_forward: the workspace is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "smooth_forward: stats is not 8-byte aligned");
    double *partials = nullptr, *mean_rows = nullptr;
    carve_smooth(workspace, a->n_rows, a->H, a->W, &partials, &mean_rows);
    HIP_TRY(launch_smooth_fwd(*a, partials, mean_rows, loss, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_smooth_backward(const BagsSmooth* a, const double* stats, const float* g_loss, float* const g_field[BAGS_MAX_POSE_ROWS],
                         float* const g_weights[BAGS_MAX_POSE_ROWS], void* stream)
{
    if (const int rc = check_smooth("smooth_backward", a)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "smooth_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "smooth_backward: stats is not 8-byte aligned");
    if (!g_loss) return fail(BAGS_ERR_ARG, "smooth_backward: null g_loss");
    bool any_map = false;
    for (int v = 0; v < a->n_rows; ++v)
        any_map |= (g_field && g_field[v]) || (a->kind == BAGS_SMOOTH_DEPTH && g_weights && g_weights[v]);
    if (!any_map) return BAGS_OK;
    HIP_TRY(launch_smooth_bwd(*a, stats, g_loss, g_field, g_weights, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- gaussian_reg.hip: one record of 8 doubles per workgroup of the sums kernel
static size_t carve_gaussian_reg(void* base, int P, double** records)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* r = c.take<double>((size_t)gaussian_reg_records(P) * BAGS_GAUSSIAN_REG_STATS);
    if (records) *records = r;
    return c.used();
}

size_t bags_gaussian_reg_workspace_size(int32_t P) { return carve_gaussian_reg(nullptr, P, nullptr); }

static int check_gaussian_reg(const char* op, const BagsGaussianReg* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->P < 0) return fail(BAGS_ERR_ARG, "%s: P < 0 (got %d)", op, a->P);
    if (a->terms >> BAGS_GAUSSIAN_REG_TERMS) return fail(BAGS_ERR_ARG, "%s: unknown bits in terms 0x%x", op, a->terms);
    if (!(a->max_ratio >= 1.0f)) return fail(BAGS_ERR_ARG, "%s: max_ratio must be >= 1", op);
    if (!(a->max_scale >= 0.0f)) return fail(BAGS_ERR_ARG, "%s: max_scale must be >= 0", op);
    if (a->P > 0 && (!a->opacity_raw || !a->scaling_raw)) return fail(BAGS_ERR_ARG, "%s: null opacity_raw / scaling_raw", op);
    return BAGS_OK;
}

int bags_gaussian_reg_forward(const BagsGaussianReg* a, void* workspace, size_t workspace_bytes, float* terms, float* count, double* stats,
                              void* stream)
{
    if (const int rc = check_gaussian_reg("gaussian_reg_forward", a)) return rc;
    if (!terms || !count || !stats) return fail(BAGS_ERR_ARG, "gaussian_reg_forward: null terms / count / stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "gaussian_reg_forward: stats is not 8-byte aligned");
    const size_t need = bags_gaussian_reg_workspace_size(a->P);
    if (need > 0 && (!workspace || workspace_bytes < need))
        return fail(BAGS_ERR_SIZE, "gaussian_reg_forward: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    if (need > 0 && reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
        return fail(BAGS_ERR_ARG, "gaussian_reg_forward: the workspace is not 16-byte aligned");
    double* records = nullptr;
    if (need > 0) carve_gaussian_reg(workspace, a->P, &records);
    HIP_TRY(launch_gaussian_reg_fwd(*a, records, terms, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_gaussian_reg_backward(const BagsGaussianReg* a, const double* stats, const float* g_terms, float* g_opacity, float* g_scaling,
                               void* stream)
{
    if (const int rc = check_gaussian_reg("gaussian_reg_backward", a)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "gaussian_reg_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "gaussian_reg_backward: stats is not 8-byte aligned");
    if (!g_terms) return fail(BAGS_ERR_ARG, "gaussian_reg_backward: null g_terms");
    if ((g_opacity && g_opacity == a->opacity_raw) || (g_scaling && g_scaling == a->scaling_raw))
        return fail(BAGS_ERR_ARG, "gaussian_reg_backward: a gradient must not be its leaf");
    if (a->P == 0 || (!g_opacity && !g_scaling)) return BAGS_OK;
    HIP_TRY(launch_gaussian_reg_bwd(*a, stats, g_terms, g_opacity, g_scaling, (hipStream_t)stream));
    return BAGS_OK;
}

// ---- alpha.hip: one row of 2 doubles per workgroup of the sums kernel, view-major.  The grid is fixed, so the layout is the same for
// every call and its size is the header's constant: there is no size function
static size_t carve_alpha(void* base, double** partials)
{
    Carver c(base, false);                       // the base as given: a misaligned one is refused, not rounded
    double* p = c.take<double>((size_t)BAGS_MAX_POSE_ROWS * BAGS_ALPHA_GROUPS * BAGS_ALPHA_STATS);
    if (partials) *partials = p;
    return c.used();
}
static_assert(BAGS_ALPHA_WORKSPACE_BYTES % 256 == 0, "what the carving helper hands out is the constant of the header");

static int check_alpha(const char* op, const BagsAlpha* a)
{
    if (!a) return fail(BAGS_ERR_ARG, "%s: null struct", op);
    if (a->mode != BAGS_ALPHA_BCE && a->mode != BAGS_ALPHA_L1 && a->mode != BAGS_ALPHA_L2 && a->mode != BAGS_ALPHA_ENTROPY)
        return fail(BAGS_ERR_ARG, "%s: unknown mode %d", op, a->mode);
    if (a->n_rows < 1 || a->n_rows > BAGS_MAX_POSE_ROWS) return fail(BAGS_ERR_ARG, "%s: n_rows %d not in 1..%d", op, a->n_rows, BAGS_MAX_POSE_ROWS);
    if (a->H < 1 || a->W < 1) return fail(BAGS_ERR_ARG, "%s: empty image %dx%d", op, a->W, a->H);
    if (!depth_prior_image_ok(a->H, a->W)) return fail(BAGS_ERR_ARG, "%s: image %dx%d has 2^31 pixels or more", op, a->W, a->H);
    if (!(a->lo > 0.0f && a->lo < a->hi && a->hi < 1.0f)) return fail(BAGS_ERR_ARG, "%s: the clamp must be 0 < lo < hi < 1", op);
    for (int v = 0; v < a->n_rows; ++v) {
        if (!a->weights[v]) return fail(BAGS_ERR_ARG, "%s: null weights[%d]", op, v);
        if (a->mode != BAGS_ALPHA_ENTROPY && !a->target[v]) return fail(BAGS_ERR_ARG, "%s: null target[%d]", op, v);
    }
    return BAGS_OK;
}

int bags_alpha_forward(const BagsAlpha* a, void* workspace, size_t workspace_bytes, float* loss, float* count, double* stats, void* stream)
{
    if (const int rc = check_alpha("alpha_forward", a)) return rc;
    if (!loss || !count || !stats) return fail(BAGS_ERR_ARG, "alpha_forward: null loss / count / stats");
    const size_t need = carve_alpha(nullptr, nullptr);                    // == BAGS_ALPHA_WORKSPACE_BYTES
    if (!workspace || workspace_bytes < need)
        return fail(BAGS_ERR_ARG, "alpha_forward: needs a workspace of %zu bytes (got %zu)", need, workspace ? workspace_bytes : (size_t)0);
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(BAGS_ERR_ARG, "alpha_forward: the workspace is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "alpha_forward: stats is not 8-byte aligned");
    double* partials = nullptr;
    carve_alpha(workspace, &partials);
    HIP_TRY(launch_alpha_fwd(*a, partials, loss, count, stats, (hipStream_t)stream));
    return BAGS_OK;
}

int bags_alpha_backward(const BagsAlpha* a, const double* stats, const float* g_loss, float* const g_weights[BAGS_MAX_POSE_ROWS], void* stream)
{
    if (const int rc = check_alpha("alpha_backward", a)) return rc;
    if (!stats) return fail(BAGS_ERR_ARG, "alpha_backward: null stats");
    if (reinterpret_cast<uintptr_t>(stats) % 8 != 0) return fail(BAGS_ERR_ARG, "alpha_backward: stats is not 8-byte aligned");
    if (!g_loss) return fail(BAGS_ERR_ARG, "alpha_backward: null g_loss");
    bool any_map = false;
    for (int v = 0; v < a->n_rows; ++v) any_map |= g_weights && g_weights[v];
    if (!any_map) return BAGS_OK;
    HIP_TRY(launch_alpha_bwd(*a, stats, g_loss, g_weights, (hipStream_t)stream));
    return BAGS_OK;
}

}  // extern "C"
