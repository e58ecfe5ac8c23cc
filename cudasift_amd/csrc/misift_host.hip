// misift_host.hip — host side of libmisift.so: context, memory, launch orchestration
// and the extern "C" entry points declared in include/misift.h.
//
// Orchestration follows the reference's host code (cudaSiftH.cu:72-232) in WHAT is
// computed and in the counter protocol, not in how it is scheduled: all kernels take a
// frame dimension so a whole batch of frames goes through each pyramid level in one
// launch; nothing is allocated, uploaded or synchronised inside the launch sequence
// (taps travel as kernel arguments, counters are reset with one async memset, the only
// host<->device sync is the final count read-back).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>
#include "common.hpp"
#include "bundle_host.hpp"
#include "chain.hpp"
#include "localize_core.hpp"
#include "merge_core.hpp"
#include "pair_plan.hpp"

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

void misift_set_error(const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *misift_last_error(void) { return g_err; }

#define ARG_CHECK_IN(who, cond)                                               \
  do {                                                                        \
    if (!(cond)) {                                                            \
      misift_set_error("%s: invalid argument: %s", who, #cond);               \
      return MISIFT_EINVAL;                                                   \
    }                                                                         \
  } while (0)
#define ARG_CHECK(cond) ARG_CHECK_IN(__func__, cond)

// ------------------------------------------------------------------ roctx
// Named ranges for rocprofv3 --marker-trace / rocprof-sys: one range per entry-point call and one
// per kernel launch.  The marker library is bound at run time, and only when a profiler has already mapped it into
// the process or MISIFT_ROCTX=1 asks for it — ordinary runs pay one predictable branch per launch.
#include <dlfcn.h>
static int (*g_roctx_push)(const char *) = nullptr;
static int (*g_roctx_pop)(void) = nullptr;
static int g_roctx_state = 0;          // 0 = untried, 1 = bound, -1 = off
static void roctx_bind_once(void)
{
  g_roctx_state = -1;
  const char *names[] = {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"};
  const char *env = getenv("MISIFT_ROCTX");
  if (env && atoi(env) == 0) return;
  void *h = nullptr;
  for (const char *n : names)
    if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
  if (!h && env && atoi(env) != 0)
    for (const char *n : names)
      if (!h) h = dlopen(n, RTLD_NOW);
  if (!h) return;
  *(void **)(&g_roctx_push) = dlsym(h, "roctxRangePushA");
  *(void **)(&g_roctx_pop) = dlsym(h, "roctxRangePop");
  if (g_roctx_push && g_roctx_pop) g_roctx_state = 1;
}
static void roctx_bind(void)
{
  static std::once_flag once;          // contexts are created from several host threads (one per device)
  std::call_once(once, roctx_bind_once);
}
struct RoctxRange {
  bool on;
  explicit RoctxRange(const char *name) : on(g_roctx_state > 0) { if (on) g_roctx_push(name); }
  ~RoctxRange() { if (on) g_roctx_pop(); }
};

// --------------------------------------------------------------- profiling
struct PendingProf { int slot; hipEvent_t a, b; };
// Identity of one synchronous extraction call; a repeated call (the reference demo extracts the same image
// 1000 times, mainSift.cpp:64-69; a tracker calls with the same buffers every frame) replays a captured hipGraph.
struct CallKey {
  const void *imgs; float *scratch; void *pts;
  int src_u8, nframes, width, height, pitch, num_octaves, scale_up, max_pts, fused, texfrac, fixnum, determ, refcap, alloc_gen;
  long long frame_stride;
  float init_blur, thresh, lowest_scale;
  // field by field: the struct has padding, and plain assignment need not preserve padding bytes
  bool operator==(const CallKey &o) const
  {
    return imgs == o.imgs && scratch == o.scratch && pts == o.pts && src_u8 == o.src_u8 && nframes == o.nframes &&
           width == o.width && height == o.height && pitch == o.pitch && num_octaves == o.num_octaves &&
           scale_up == o.scale_up && max_pts == o.max_pts && fused == o.fused && texfrac == o.texfrac &&
           fixnum == o.fixnum && determ == o.determ && refcap == o.refcap && alloc_gen == o.alloc_gen && frame_stride == o.frame_stride &&
           init_blur == o.init_blur && thresh == o.thresh && lowest_scale == o.lowest_scale;
  }
};
struct CtxExtra {
  std::vector<PendingProf> pending;
  std::vector<hipEvent_t> pool;
  // hipGraph replay of the launch sequence of misift_extract_enqueue (launch-latency bound for a single frame)
  int graph_mode = 0;                 // off by default (measured slower, see misift.h); MISIFT_GRAPH=1 / misift_ctx_set_graph_replay
  bool have_last = false, have_graph = false;
  CallKey last_key, graph_key;
  hipGraphExec_t gexec = nullptr;
  hipStream_t gstream = nullptr;      // capture / replay stream (capture is not allowed on the null stream)
  hipEvent_t gev_in = nullptr, gev_out = nullptr;
  // batches in flight (misift_ctx_set_batches_in_flight): K child contexts = K in-order pipelines (stream, counters,
  // candidate lists, detection staging each) that misift_extract_batch_packed_async rotates over
  std::vector<misift_ctx *> lanes;
  std::vector<hipEvent_t> lane_done;   // 2K events: done[ticket % 2K] is recorded behind batch `ticket` on its lane's stream
  hipEvent_t ev_in = nullptr;          // recorded on the caller's stream at every call: the lane starts behind it
  hipEvent_t ev_single = nullptr;      // K = 1: misift_ctx_wait_batch records this one on the context stream
  hipEvent_t ev_switch = nullptr;      // misift_ctx_set_stream: recorded on the old stream, waited for on the new one
  unsigned long long ticket = 0;
  misift_ctx *last_lane = nullptr;     // the pipeline that took the most recent batch (nullptr: the context itself)
  hipEvent_t last_done = nullptr;
  hipStream_t own_stream = nullptr;    // a child context owns its stream
  std::vector<std::pair<std::string, double>> knobs;   // misift_test_set_knob calls so far: replayed on pipelines built later
  // host-side tap tables of the last call's (num_octaves, init_blur)
  int taps_noct = -1;
  float taps_table[8 * 12 * 16];
  float k9_blur = -1.0f, k9[9], k5[5];
  bool k5_done = false;
  // misift_match_batch and misift_*_homography_batch: pinned copies of the callers' pair / frame / seed lists, a ring of
  // MB_RING slots (a slot is refilled once the call that last used it has run: mb_done), and misift_match_batch's device
  // plan (header + one PairPlan per pair)
  static const int MB_RING = 4;
  int *mb_pairs[MB_RING] = {};
  size_t mb_pairs_cap[MB_RING] = {};
  hipEvent_t mb_done[MB_RING] = {};
  unsigned mb_next = 0;
  void *d_mb_plan = nullptr;
  size_t mb_plan_bytes = 0;
};
static CtxExtra *extra(misift_ctx *ctx);

LaunchScope::LaunchScope(misift_ctx *c, const char *n) : ctx(c), name(n)
{
  if (g_roctx_state > 0) g_roctx_push(n);
  if (ctx->profile) {
    CtxExtra *x = extra(ctx);
    hipEvent_t a, b;
    if (x->pool.size() >= 2) {
      a = x->pool.back(); x->pool.pop_back();
      b = x->pool.back(); x->pool.pop_back();
    } else {
      hipEventCreate(&a);
      hipEventCreate(&b);
    }
    int slot = -1;
    for (int i = 0; i < ctx->nprof; i++)
      if (!strcmp(ctx->prof[i].name, n)) slot = i;
    if (slot < 0 && ctx->nprof < 32) {
      slot = ctx->nprof++;
      strncpy(ctx->prof[slot].name, n, 31);
      ctx->prof[slot].name[31] = 0;
      ctx->prof[slot].total_ms = 0;
      ctx->prof[slot].calls = 0;
    }
    hipEventRecord(a, ctx->stream);
    x->pending.push_back({slot, a, b});
  }
}

int LaunchScope::finish()
{
  if (g_roctx_state > 0) g_roctx_pop();
  if (ctx->profile) {
    CtxExtra *x = extra(ctx);
    hipEventRecord(x->pending.back().b, ctx->stream);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    misift_set_error("launch of %s failed: %s", name, hipGetErrorString(e));
    return MISIFT_EHIP;
  }
  return MISIFT_OK;
}

static int resolve_profile(misift_ctx *ctx)
{
  CtxExtra *x = extra(ctx);
  if (x->pending.empty()) return MISIFT_OK;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (auto &p : x->pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess && p.slot >= 0) {
      ctx->prof[p.slot].total_ms += ms;
      ctx->prof[p.slot].calls++;
    }
    x->pool.push_back(p.a);
    x->pool.push_back(p.b);
  }
  x->pending.clear();
  return MISIFT_OK;
}

// ----------------------------------------------------------------- context
struct CtxFull {
  misift_ctx c;
  CtxExtra x;
};
static CtxExtra *extra(misift_ctx *ctx) { return &reinterpret_cast<CtxFull *>(ctx)->x; }

// MISIFT_DEVICES="2,3" (SURVEY section 5): device i of this library = HIP device list[i], the others do not exist for
// it — like HIP_VISIBLE_DEVICES but for libmisift.so only (a process that shares the GPUs with another runtime keeps
// its own numbering).  Unset or empty: every HIP device, identity.  Read once.
static std::vector<int> build_device_map(void)
{
  std::vector<int> m;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  const char *e = getenv("MISIFT_DEVICES");
  if (e && *e) {
    for (const char *p = e; *p;) {
      char *end = nullptr;
      const long d = strtol(p, &end, 10);
      if (end == p) break;
      if (d >= 0 && d < n) m.push_back((int)d);
      p = (*end == ',') ? end + 1 : end;
      if (*end && *end != ',') break;
    }
  } else {
    for (int i = 0; i < n; i++) m.push_back(i);
  }
  return m;
}
static const std::vector<int> &device_map(void)
{
  // C++11 magic static: built exactly once even when several host threads create their contexts at the same time
  // (one thread per device is how the multi-GPU entry points are meant to be driven)
  static const std::vector<int> m = build_device_map();
  return m;
}
static int physical_device(int logical)
{
  const std::vector<int> &m = device_map();
  return (logical >= 0 && logical < (int)m.size()) ? m[(size_t)logical] : -1;
}

extern "C" int misift_device_count(void) { return (int)device_map().size(); }

extern "C" int misift_device_info(int device, char *name, int name_len, int *mem_clock_khz, int *bus_width_bits,
                                  size_t *total_mem_bytes, int *num_cus, int *lds_bytes_per_block)
{
  ARG_CHECK(physical_device(device) >= 0);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, physical_device(device)));
  if (name && name_len > 0) {
    // ROCm 7.2 leaves prop.name empty for some Instinct parts: fall back to the ISA name
    if (prop.name[0]) snprintf(name, name_len, "%s", prop.name);
    else snprintf(name, name_len, "AMD Instinct (%s)", prop.gcnArchName);
  }
  if (mem_clock_khz) *mem_clock_khz = prop.memoryClockRate;
  if (bus_width_bits) *bus_width_bits = prop.memoryBusWidth;
  if (total_mem_bytes) *total_mem_bytes = prop.totalGlobalMem;
  if (num_cus) *num_cus = prop.multiProcessorCount;
  if (lds_bytes_per_block) *lds_bytes_per_block = (int)prop.sharedMemPerBlock;
  return MISIFT_OK;
}

extern "C" int misift_device_arch(int device, char *arch, int arch_len)
{
  ARG_CHECK(arch && arch_len > 0 && physical_device(device) >= 0);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, physical_device(device)));
  snprintf(arch, arch_len, "%s", prop.gcnArchName);
  return MISIFT_OK;
}

#undef misift_default_options
static void default_options_full(misift_options *opt);
extern "C" void misift_default_options_sized(misift_options *opt, size_t struct_size)
{
  if (!opt) return;
  misift_options o;
  default_options_full(&o);
  memcpy(opt, &o, struct_size < sizeof(o) ? struct_size : sizeof(o));
}
extern "C" void misift_default_options(misift_options *opt)      // binaries built against the r04 header: its seven fields
{
  misift_default_options_sized(opt, 7 * sizeof(int));
}
static void default_options_full(misift_options *opt)
{
  memset(opt, 0, sizeof(*opt));
  opt->texfrac_bits = 8;
  opt->fix_numpts = 0;
  opt->match_full = 0;
  opt->match_exact_top2 = 0;
  opt->quiet = 0;
  opt->fused = 1;
  const char *e;
  if ((e = getenv("MISIFT_TEXFRAC_BITS"))) opt->texfrac_bits = atoi(e);
  if ((e = getenv("MISIFT_FIX_NUMPTS"))) opt->fix_numpts = atoi(e);
  if ((e = getenv("MISIFT_MATCH_FULL"))) opt->match_full = atoi(e);
  if ((e = getenv("MISIFT_MATCH_EXACT_TOP2"))) opt->match_exact_top2 = atoi(e);
  if ((e = getenv("MISIFT_QUIET"))) opt->quiet = atoi(e);
  if ((e = getenv("MISIFT_FUSED"))) opt->fused = atoi(e);
  if ((e = getenv("MISIFT_DETERMINISTIC"))) opt->deterministic = atoi(e) != 0;
  opt->reference_cap = 0;
  if ((e = getenv("MISIFT_REFERENCE_CAP"))) opt->reference_cap = atoi(e) != 0;
}

// ---- developer / test knobs (launch shapes, path selection).  ONE table: knob name <-> the environment variable that sets it
// when MISIFT_TUNABLES=1.  README.md lists them; tests/test_cabi_cpu.py checks that list against this table.
struct KnobName { const char *name, *env; };
static const KnobName KNOBS[] = {
  {"graph", "MISIFT_GRAPH"}, {"split_tail", "MISIFT_SPLIT_TAIL"}, {"bin", "MISIFT_BIN"}, {"descr_occ", "MISIFT_DESCR_OCC"},
  {"tile", "MISIFT_TILE"}, {"tile_descr", "MISIFT_TILE_DESCR"}, {"tile_orient", "MISIFT_TILE_ORIENT"},
  {"orient_blocks", "MISIFT_ORIENT_BLOCKS"}, {"point_blocks", "MISIFT_POINT_BLOCKS"}, {"strip_waves", "MISIFT_STRIP_WAVES"},
  {"scan_waves", "MISIFT_SCAN_WAVES"}, {"chain_frames", "MISIFT_CHAIN_FRAMES"}, {"chain_embed", "MISIFT_CHAIN_EMBED"},
  {"chain_wait_us", "MISIFT_CHAIN_WAIT_US"}, {"bin_min_frames", "MISIFT_BIN_MIN_FRAMES"}, {"small_frames", "MISIFT_SMALL_FRAMES"},
  {"balance", "MISIFT_BALANCE"}, {"fold_tail", "MISIFT_FOLD_TAIL"}, {"patch_reach", "MISIFT_TEST_PATCH_REACH"},
  {"lds_pad_lpd", "MISIFT_LDS_PAD_LPD"}, {"lds_pad_scan", "MISIFT_LDS_PAD_SCAN"}, {"lds_pad_orient", "MISIFT_LDS_PAD_ORIENT"},
  {"lds_pad_descr", "MISIFT_LDS_PAD_DESCR"}, {"lowpass_tile", "MISIFT_LOWPASS_TILE"}, {"strip_rows_small", "MISIFT_STRIP_ROWS_SMALL"},
  {"scan_rows_small_coarse", "MISIFT_SCAN_ROWS_SMALL_COARSE"}, {"scan_rows_small", "MISIFT_SCAN_ROWS_SMALL"},
  {"host_spin", "MISIFT_HOST_SPIN"}, {"refcap_limit", "MISIFT_TEST_REFCAP_LIMIT"}, {"fuse_orient", "MISIFT_FUSE_ORIENT"},
  {"fuse_wait_us", "MISIFT_FUSE_WAIT_US"},
};
static bool tunables_from_env()
{
  const char *e = getenv("MISIFT_TUNABLES");
  return e && atoi(e) != 0;
}
static int apply_knob(misift_ctx *ctx, const char *name, double v)
{
  const int i = (int)v;
  const auto is = [&](const char *n) { return strcmp(name, n) == 0; };
  if (is("graph")) extra(ctx)->graph_mode = i != 0;
  else if (is("split_tail")) ctx->split_tail = i;
  else if (is("bin")) ctx->bin_detections = i != 0;
  else if (is("descr_occ")) ctx->descr_occ = i;
  else if (is("tile")) ctx->tile_descr = ctx->tile_orient = i != 0;
  else if (is("tile_descr")) ctx->tile_descr = i != 0;
  else if (is("tile_orient")) ctx->tile_orient = i != 0;
  else if (is("orient_blocks")) ctx->orient_blocks_per_cu = i > 0 ? i : 6;
  else if (is("point_blocks")) ctx->point_blocks_per_cu = i > 0 ? i : 8;
  else if (is("strip_waves")) ctx->strip_waves_per_cu = i > 0 ? i : 16;
  else if (is("scan_waves")) ctx->scan_waves_per_cu = i > 0 ? i : 16;
  else if (is("chain_frames")) ctx->chain_max_frames = i;
  else if (is("chain_embed")) ctx->chain_embed = i != 0;
  else if (is("chain_wait_us")) ctx->chain_wait_ticks = (unsigned)(v * 100.0);
  else if (is("bin_min_frames")) ctx->bin_min_frames = i;
  else if (is("small_frames")) ctx->small_frames = i;
  else if (is("balance")) ctx->balance_frames = i != 0;
  else if (is("fold_tail")) ctx->fold_descr_tail = i != 0;
  else if (is("patch_reach")) { if (v > 0.0 && v < 17.9) ctx->patch_reach = (float)v; else if (v >= 17.9) ctx->patch_reach = 17.9f; }
  else if (is("lds_pad_lpd")) ctx->lds_pad_lpd = i;
  else if (is("lds_pad_scan")) ctx->lds_pad_scan = i;
  else if (is("lds_pad_orient")) ctx->lds_pad_orient = i;
  else if (is("lds_pad_descr")) ctx->lds_pad_descr = i;
  else if (is("lowpass_tile")) ctx->lowpass_tile = i != 0;
  else if (is("strip_rows_small")) ctx->strip_rows_small = i >= 2 ? i / 2 * 2 : 6;
  else if (is("scan_rows_small_coarse")) ctx->scan_rows_small_coarse = i > 0 ? i : 2;
  else if (is("scan_rows_small")) ctx->scan_rows_small = i > 0 ? i : 4;
  else if (is("host_spin")) ctx->host_spin = i != 0;
  else if (is("refcap_limit")) ctx->refcap_limit = i >= 0 && i <= 240 ? i : 32;
  else if (is("fuse_orient")) ctx->fuse_orient = i != 0;
  else if (is("fuse_wait_us")) ctx->fuse_wait_ticks = (unsigned)(v * 100.0);
  else { misift_set_error("misift_test_set_knob: unknown knob '%s'", name); return MISIFT_EINVAL; }
  return MISIFT_OK;
}
// Test / tuning entry point: set one knob of this context (and of its pipelines behind misift_ctx_set_batches_in_flight).
// name = NULL: *names_out (optional) receives the comma-separated list "knob=ENV,..." of everything there is.
extern "C" int misift_test_set_knob(misift_ctx *ctx, const char *name, double value);
extern "C" const char *misift_test_knob_names(void)
{
  static std::string all;
  if (all.empty())
    for (const KnobName &k : KNOBS) all += std::string(all.empty() ? "" : ",") + k.name + "=" + k.env;
  return all.c_str();
}

extern "C" void misift_ctx_destroy(misift_ctx *ctx);
// Everything misift_ctx_create sets up after `new CtxFull()`; on any failure the caller destroys the
// half-built context (misift_ctx_destroy tolerates null members), so nothing leaks.
static int ctx_init(misift_ctx *ctx, CtxFull *f, int device, void *stream)
{
  ctx->device = device;
  ctx->stream = (hipStream_t)stream;
  default_options_full(&ctx->opt);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  ctx->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // ---- launch shapes and path selection: DEFAULTS ONLY.  The developer / test knobs that change them are applied by
  // apply_knob() — through misift_test_set_knob, or from the environment when MISIFT_TUNABLES=1 (tools/, the variant runs of
  // the test suite); a production process reads none of those variables (r06: they were 30 getenv calls right here).
  // work decomposition of the streaming kernels: wavefronts aimed at per CU and launch
  ctx->strip_waves_per_cu = 32;   // measured: lowpass_down 0.247 -> 0.220 ms vs 16 (better balance over the CUs, 64-row segments)
  ctx->scan_waves_per_cu = 32;
  ctx->split_tail = 8;            // batches of >= 8 frames: measured +2.8 % frames/s (0 disables, N sets the smallest batch;
                                  // a single frame is launch-latency bound and loses)
  {
    int lo = 0, hi = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
    HIP_TRY(hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, hi));
    HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  }
  ctx->bin_detections = 1;
  ctx->descr_occ = 4;
  ctx->tile_descr = 1;
  ctx->tile_orient = 0;
  ctx->orient_blocks_per_cu = 6;          // one round of resident workgroups: orient_all runs 6 waves/SIMD (r06; 5 before)
  ctx->point_blocks_per_cu = 8;
  ctx->chain_max_frames = 4;
  ctx->chain_embed = 1;
  ctx->chain_wait_ticks = 10000000u;          // 100 ms of the 100 MHz wall clock: ~4 orders of magnitude above the chain's own time
  ctx->bin_min_frames = 4;
  ctx->small_frames = 4;
  ctx->balance_frames = 1;       // r05: on by default (full GPU suite + bench A/B both ways: profiles/r05_balance_*); 0 restores per-frame grids
  ctx->fold_descr_tail = 1;
  ctx->fuse_orient = 0;                       // r06: a single call's orientations + descriptors as ONE launch — built, parity-green,
                                              // and 12-30 us SLOWER than the two launches: off
  ctx->fuse_wait_ticks = 10000000u;           // 100 ms, like the chain's
  ctx->patch_reach = 17.9f;                   // = PATCH_REACH of kernels_points.hip: what the LDS window of descr_all covers
  ctx->refcap_limit = 32;                     // MEMWID of FindPointsMultiNew (tests lower it so that natural frames reach it)
  ctx->lowpass_tile = 1;
  ctx->strip_rows_small = 6;
  // (r04 sweep, profiles/r04_single_call_sweep_step5.txt: fine / coarse rows 9/9 31.0 us, 9/4 25.2, 6/4 23.2, 4/3 21.8, 4/2 21.2, 3/3 22.5)
  ctx->scan_rows_small_coarse = 2;
  ctx->scan_rows_small = 4;
  // 0 = a synchronous call returns after hipStreamSynchronize (everything the call wrote is complete and visible to any
  // stream, device or host copy: the reference's contract).  1 = it returns as soon as the last kernel's flag reaches
  // pinned host memory (opt-in: misift_ctx_set_early_return; the cudaSift.h shim does, its read-back is same-stream).
  ctx->host_spin = 0;
  if (tunables_from_env()) {
    for (const KnobName &k : KNOBS)
      if (const char *e = getenv(k.env)) apply_knob(ctx, k.name, atof(e));
  }
  HIP_TRY(hipEventCreate(&ctx->ev0));
  HIP_TRY(hipEventCreate(&ctx->ev1));
  HIP_TRY(misift_dev_alloc((void **)&ctx->d_flags, sizeof(unsigned) * 64, "flags"));
  HIP_TRY(hipMemsetAsync(ctx->d_flags, 0, sizeof(unsigned) * 64, ctx->stream));
  HIP_TRY(hipHostMalloc((void **)&ctx->h_flags, sizeof(unsigned) * 64, hipHostMallocDefault));
  memset(ctx->h_flags, 0, sizeof(unsigned) * 64);
  int rc = misift_ensure_frames(ctx, 1, 65536);
  if (rc) return rc;
  return launch_selftest(ctx);
}

static int ctx_create_physical(int device, void *stream, bool own_stream, misift_ctx **out)
{
  HIP_TRY(hipSetDevice(device));
  CtxFull *f = new CtxFull();
  misift_ctx *ctx = &f->c;
  memset(ctx, 0, sizeof(*ctx));
  if (own_stream) {
    hipStream_t s = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e != hipSuccess) {
      misift_set_error("hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
      delete f;
      return MISIFT_EHIP;
    }
    f->x.own_stream = s;
    stream = s;
  }
  const int rc = ctx_init(ctx, f, device, stream);
  if (rc) {
    misift_ctx_destroy(ctx);                            // keeps the error message of the failing step
    return rc;
  }
  *out = ctx;
  return MISIFT_OK;
}

extern "C" int misift_ctx_set_batches_in_flight(misift_ctx *ctx, int k);

extern "C" int misift_ctx_create(int device, void *stream, misift_ctx **out)
{
  ARG_CHECK(out != nullptr);
  *out = nullptr;
  roctx_bind();
  int n = misift_device_count();
  if (n <= 0) {
    misift_set_error("no HIP device visible");
    return MISIFT_ENODEV;
  }
  if (device < 0 || device >= n) device = n - 1;      // like InitCuda: clamp (cudaSiftH.cu:27)
  device = physical_device(device);                   // MISIFT_DEVICES: from here on the HIP device number
  int rc = ctx_create_physical(device, stream, false, out);
  if (rc) return rc;
  if (const char *e = getenv("MISIFT_BATCHES_IN_FLIGHT")) {
    const int k = atoi(e);
    if (k < 1 || k > 8) {                       // a bad value must not make context creation fail
      if (!getenv("MISIFT_QUIET")) fprintf(stderr, "misift: warning: MISIFT_BATCHES_IN_FLIGHT=%s ignored (1..8)\n", e);
    } else {
      rc = misift_ctx_set_batches_in_flight(*out, k);
      if (rc) { misift_ctx_destroy(*out); *out = nullptr; }
    }
  }
  return rc;
}

// ---- batches in flight: an in-context ring of pipelines
// One misift_ctx is ONE in-order pipeline: batch k+1 starts when batch k is done, so the HBM-bound front end of a batch
// (lowpass_down, 0.24 ms at 0.7 of the HBM peak) never runs beside the VALU-bound kernels of another and every launch
// tail leaves CUs idle.  With K > 1 the context owns K child pipelines (own stream, counters, candidate lists, detection
// staging each — the caller rotates >= K scratch arenas and output buffers) and misift_extract_batch_packed_async hands
// consecutive calls to consecutive pipelines: r02 measured +8-9 % frames/s for K = 3-4 with separate contexts
// (bench.py --contexts); this is the same thing behind ONE context.  The caller's stream only carries a marker per
// call (the batch starts behind everything enqueued on it before the call); completion is observed through
// misift_ctx_wait_batch / misift_gather_post / misift_ctx_sync — NOT through the caller's stream.
extern "C" int misift_ctx_set_batches_in_flight(misift_ctx *ctx, int k)
{
  ARG_CHECK(ctx != nullptr && k >= 1 && k <= 8);
  CtxExtra *x = extra(ctx);
  HIP_TRY(hipSetDevice(ctx->device));
  // drain and drop the current ring first
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (misift_ctx *l : x->lanes) { hipStreamSynchronize(l->stream); misift_ctx_destroy(l); }
  x->lanes.clear();
  for (hipEvent_t e : x->lane_done) hipEventDestroy(e);
  x->lane_done.clear();
  x->last_lane = nullptr; x->last_done = nullptr; x->ticket = 0;
  if (k == 1) return MISIFT_OK;
  // build the whole ring or none of it: a half-built ring must never be visible to misift_extract_batch_packed_async
  std::vector<misift_ctx *> lanes;
  std::vector<hipEvent_t> done;
  int rc = MISIFT_OK;
  if (!x->ev_in && hipEventCreateWithFlags(&x->ev_in, hipEventDisableTiming) != hipSuccess) rc = MISIFT_EHIP;
  for (int i = 0; i < k && !rc; i++) {
    misift_ctx *l = nullptr;
    rc = ctx_create_physical(ctx->device, nullptr, true, &l);
    if (!rc) {
      lanes.push_back(l);
      for (const auto &kv : x->knobs) apply_knob(l, kv.first.c_str(), kv.second);
    }
  }
  for (int i = 0; i < 2 * k && !rc; i++) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      misift_set_error("hipEventCreateWithFlags failed while building %d pipelines", k);
      rc = MISIFT_EHIP;
    } else {
      done.push_back(e);
    }
  }
  if (rc) {
    for (misift_ctx *l : lanes) misift_ctx_destroy(l);
    for (hipEvent_t e : done) hipEventDestroy(e);
    return rc;                                        // the context stays a plain in-order one
  }
  x->lanes.swap(lanes);
  x->lane_done.swap(done);
  return MISIFT_OK;
}

extern "C" int misift_test_set_knob(misift_ctx *ctx, const char *name, double value)
{
  ARG_CHECK(ctx != nullptr && name != nullptr);
  int rc = apply_knob(ctx, name, value);
  if (rc) return rc;
  CtxExtra *x = extra(ctx);
  x->knobs.emplace_back(name, value);
  for (misift_ctx *l : x->lanes) apply_knob(l, name, value);
  return MISIFT_OK;
}

extern "C" int misift_ctx_set_early_return(misift_ctx *ctx, int on)
{
  ARG_CHECK(ctx != nullptr);
  if (!(tunables_from_env() && getenv("MISIFT_HOST_SPIN"))) ctx->host_spin = on ? 1 : 0;     // A/B runs: the environment has the last word
  return MISIFT_OK;
}

extern "C" int misift_ctx_last_call_balanced(misift_ctx *ctx) { return ctx ? ctx->cur_balanced : -1; }

extern "C" int misift_ctx_descr_big_fallbacks(misift_ctx *ctx) { return ctx ? ctx->descr_big_fallbacks : -1; }

extern "C" int misift_ctx_chain_fallbacks(misift_ctx *ctx) { return ctx ? ctx->chain_fallbacks : -1; }
extern "C" int misift_ctx_fuse_fallbacks(misift_ctx *ctx) { return ctx ? ctx->fuse_fallbacks : -1; }

extern "C" int misift_ctx_get_batches_in_flight(misift_ctx *ctx)
{
  return ctx ? (extra(ctx)->lanes.empty() ? 1 : (int)extra(ctx)->lanes.size()) : 0;
}

// The pipeline that holds the results (counters, profile) of the most recent batch, and the stream it ran on.
static misift_ctx *result_ctx(misift_ctx *ctx)
{
  CtxExtra *x = extra(ctx);
  return x->last_lane ? x->last_lane : ctx;
}
hipStream_t misift_ctx_result_stream(misift_ctx *ctx) { return result_ctx(ctx)->stream; }

// Record a caller-owned hipEvent_t behind the most recently enqueued batch of `ctx` (on the stream that batch runs on).
// Unlike misift_ctx_wait_batch this adds no waiting stream: on a GPU whose hardware queues are oversubscribed a waiting
// side stream can share a queue with a pipeline and hold it up.
extern "C" int misift_ctx_record_batch(misift_ctx *ctx, void *hip_event)
{
  ARG_CHECK(ctx != nullptr && hip_event != nullptr);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipEventRecord((hipEvent_t)hip_event, result_ctx(ctx)->stream));
  return MISIFT_OK;
}

// `stream` waits for the most recently enqueued batch of `ctx` (any K; with K = 1 the same as an event recorded on the
// context stream now).
extern "C" int misift_ctx_wait_batch(misift_ctx *ctx, void *stream)
{
  ARG_CHECK(ctx != nullptr);
  CtxExtra *x = extra(ctx);
  HIP_TRY(hipSetDevice(ctx->device));
  if (x->last_done) {
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, x->last_done, 0));
    return MISIFT_OK;
  }
  if ((hipStream_t)stream == ctx->stream) return MISIFT_OK;
  if (!x->ev_single) HIP_TRY(hipEventCreateWithFlags(&x->ev_single, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(x->ev_single, ctx->stream));
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, x->ev_single, 0));
  return MISIFT_OK;
}

extern "C" void misift_ctx_destroy(misift_ctx *ctx)
{
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  CtxExtra *x = extra(ctx);
  for (misift_ctx *l : x->lanes) misift_ctx_destroy(l);
  x->lanes.clear();
  for (hipEvent_t e : x->lane_done) hipEventDestroy(e);
  if (x->ev_in) hipEventDestroy(x->ev_in);
  if (x->ev_single) hipEventDestroy(x->ev_single);
  if (x->ev_switch) hipEventDestroy(x->ev_switch);
  if (x->gexec) hipGraphExecDestroy(x->gexec);
  if (x->gstream) { hipStreamSynchronize(x->gstream); hipStreamDestroy(x->gstream); }
  if (x->gev_in) hipEventDestroy(x->gev_in);
  if (x->gev_out) hipEventDestroy(x->gev_out);
  for (auto &p : x->pending) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto e : x->pool) hipEventDestroy(e);
  for (int i = 0; i < CtxExtra::MB_RING; i++) {
    if (x->mb_done[i]) hipEventDestroy(x->mb_done[i]);
    if (x->mb_pairs[i]) hipHostFree(x->mb_pairs[i]);
  }
  if (x->d_mb_plan) misift_dev_free(x->d_mb_plan);
  if (ctx->d_counters) misift_dev_free(ctx->d_counters);
  if (ctx->h_counters) hipHostFree(ctx->h_counters);
  if (ctx->d_flags) misift_dev_free(ctx->d_flags);
  if (ctx->h_flags) hipHostFree(ctx->h_flags);
  if (ctx->d_cand) misift_dev_free(ctx->d_cand);
  if (ctx->d_det) misift_dev_free(ctx->d_det);
  if (ctx->d_det_sorted) misift_dev_free(ctx->d_det_sorted);
  if (ctx->d_block_map) misift_dev_free(ctx->d_block_map);
  if (ctx->d_own_scratch) misift_dev_free(ctx->d_own_scratch);
  if (ctx->d_match_tmp) misift_dev_free(ctx->d_match_tmp);
  if (ctx->d_refcap) misift_dev_free(ctx->d_refcap);
  if (ctx->d_capcnt) misift_dev_free(ctx->d_capcnt);
  if (ctx->ev0) hipEventDestroy(ctx->ev0);
  if (ctx->ev1) hipEventDestroy(ctx->ev1);
  if (ctx->stream2) { hipStreamSynchronize(ctx->stream2); hipStreamDestroy(ctx->stream2); }
  if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
  if (x->own_stream) hipStreamDestroy(x->own_stream);
  delete reinterpret_cast<CtxFull *>(ctx);
}

extern "C" int misift_ctx_set_graph_replay(misift_ctx *ctx, int on)
{
  ARG_CHECK(ctx != nullptr);
  extra(ctx)->graph_mode = on ? 1 : 0;
  return MISIFT_OK;
}

extern "C" int misift_ctx_set_stream(misift_ctx *ctx, void *stream)
{
  ARG_CHECK(ctx != nullptr);
  hipStream_t to = (hipStream_t)stream;
  if (to == ctx->stream) return MISIFT_OK;
  // The context stays one in-order pipeline: its temp, its pair plan, its pinned ring and its counters are not tied to a
  // stream, so the new stream starts behind everything enqueued through the context on the old one.  No host wait.
  CtxExtra *x = extra(ctx);
  HIP_TRY(hipSetDevice(ctx->device));
  if (!x->ev_switch) HIP_TRY(hipEventCreateWithFlags(&x->ev_switch, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(x->ev_switch, ctx->stream));
  HIP_TRY(hipStreamWaitEvent(to, x->ev_switch, 0));
  ctx->stream = to;
  return MISIFT_OK;
}

extern "C" int misift_ctx_sync(misift_ctx *ctx)
{
  ARG_CHECK(ctx != nullptr);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (misift_ctx *l : extra(ctx)->lanes) HIP_TRY(hipStreamSynchronize(l->stream));
  return MISIFT_OK;
}

#undef misift_set_options
#undef misift_get_options
#define MISIFT_OPTIONS_R04_BYTES (7 * sizeof(int))       // texfrac_bits ... deterministic: the struct of the r04 header
extern "C" int misift_set_options_sized(misift_ctx *ctx, const misift_options *opt, size_t struct_size)
{
  ARG_CHECK(ctx && opt && struct_size >= sizeof(int) && struct_size % sizeof(int) == 0);
  misift_options o = ctx->opt;                                   // fields the caller's header does not have keep their value
  memcpy(&o, opt, struct_size < sizeof(o) ? struct_size : sizeof(o));
  ARG_CHECK(o.texfrac_bits == 8 || o.texfrac_bits == 23 || o.texfrac_bits == 0);
  ctx->opt = o;
  return MISIFT_OK;
}

extern "C" int misift_get_options_sized(misift_ctx *ctx, misift_options *opt, size_t struct_size)
{
  ARG_CHECK(ctx && opt && struct_size >= sizeof(int));
  memcpy(opt, &ctx->opt, struct_size < sizeof(ctx->opt) ? struct_size : sizeof(ctx->opt));
  return MISIFT_OK;
}

// the symbols binaries built against the r04 header call: its seven fields, nothing behind them
extern "C" int misift_set_options(misift_ctx *ctx, const misift_options *opt)
{
  return misift_set_options_sized(ctx, opt, MISIFT_OPTIONS_R04_BYTES);
}

extern "C" int misift_get_options(misift_ctx *ctx, misift_options *opt)
{
  return misift_get_options_sized(ctx, opt, MISIFT_OPTIONS_R04_BYTES);
}

int misift_ensure_frames(misift_ctx *ctx, int nframes, size_t cand_cap)
{
  if (nframes > ctx->cap_frames) {
    if (ctx->d_counters) HIP_TRY(misift_dev_free(ctx->d_counters));
    if (ctx->h_counters) HIP_TRY(hipHostFree(ctx->h_counters));
    ctx->d_counters = nullptr; ctx->h_counters = nullptr;
    // (CNT_SPARE_BLOCKS more than frames: the call's flags and ticket words live behind the last frame's counters)
    HIP_TRY(misift_dev_alloc((void **)&ctx->d_counters, sizeof(unsigned) * CNT_STRIDE * ((size_t)nframes + CNT_SPARE_BLOCKS), "counters"));
    ctx->alloc_gen++;
    // one block more than frames: the word behind the last frame's counters is the host-export flag (descr_big_kernel)
    HIP_TRY(hipHostMalloc((void **)&ctx->h_counters, sizeof(unsigned) * CNT_STRIDE * ((size_t)nframes + 1), hipHostMallocDefault));
    HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned) * CNT_STRIDE * ((size_t)nframes + CNT_SPARE_BLOCKS), ctx->stream));
    memset(ctx->h_counters, 0, sizeof(unsigned) * CNT_STRIDE * ((size_t)nframes + 1));
  }
  if (nframes > ctx->cap_frames || cand_cap > ctx->cand_cap) {
    const int nf = nframes > ctx->cap_frames ? nframes : ctx->cap_frames;
    const size_t cc = cand_cap > ctx->cand_cap ? cand_cap : ctx->cand_cap;
    if (ctx->d_cand) HIP_TRY(misift_dev_free(ctx->d_cand));
    ctx->d_cand = nullptr;
    HIP_TRY(misift_dev_alloc((void **)&ctx->d_cand, sizeof(unsigned) * cc * nf, "candidates"));
    ctx->alloc_gen++;
    ctx->cand_cap = cc;
    ctx->cap_frames = nf;
  }
  return MISIFT_OK;
}

// grow-only temporary device buffer shared by the matcher (chunk partials) and the homography search
int misift_ensure_tmp(misift_ctx *ctx, size_t bytes)
{
  if (bytes > ctx->match_tmp_bytes) {
    if (ctx->d_match_tmp) {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      HIP_TRY(misift_dev_free(ctx->d_match_tmp));
    }
    ctx->d_match_tmp = nullptr; ctx->match_tmp_bytes = 0;
    HIP_TRY(misift_dev_alloc(&ctx->d_match_tmp, bytes, "match_tmp"));
    ctx->match_tmp_bytes = bytes;
  }
  return MISIFT_OK;
}

static int ensure_det(misift_ctx *ctx, int nframes, int max_pts)
{
  if (nframes > ctx->cap_det_frames || max_pts > ctx->det_max_pts) {
    const int nf = nframes > ctx->cap_det_frames ? nframes : ctx->cap_det_frames;
    const int mp = max_pts > ctx->det_max_pts ? max_pts : ctx->det_max_pts;
    if (ctx->d_det) HIP_TRY(misift_dev_free(ctx->d_det));
    if (ctx->d_det_sorted) HIP_TRY(misift_dev_free(ctx->d_det_sorted));
    ctx->d_det = nullptr; ctx->d_det_sorted = nullptr; ctx->cap_det_frames = 0; ctx->det_max_pts = 0;
    HIP_TRY(misift_dev_alloc((void **)&ctx->d_det, sizeof(Detection) * (size_t)nf * MISIFT_MAX_OCTAVES * mp, "detections"));
    HIP_TRY(misift_dev_alloc((void **)&ctx->d_det_sorted, sizeof(Detection) * (size_t)nf * MISIFT_MAX_OCTAVES * mp, "detections_binned"));
    ctx->alloc_gen++;
    ctx->cap_det_frames = nf;
    ctx->det_max_pts = mp;
  }
  return MISIFT_OK;
}

// ------------------------------------------------------------------ memory
// ---- guard mode (test infrastructure inside the product library; inert unless switched on)
#define GUARD_BAND_BYTE 0xA5
#define GUARD_POISON_BYTE 0xFF
struct GuardRec { char *base; size_t bytes; char tag[24]; };
static std::mutex g_guard_mu;
static std::map<void *, GuardRec> g_guard_map;
static int g_guard_mode = -1;                  // -1: not decided yet (MISIFT_GUARD is read at the first allocation)
static bool guard_on()
{
  if (g_guard_mode < 0) {
    const char *e = getenv("MISIFT_GUARD");
    g_guard_mode = (e && atoi(e) != 0) ? 1 : 0;
  }
  return g_guard_mode == 1;
}
hipError_t misift_dev_alloc(void **out, size_t bytes, const char *tag)
{
  if (!guard_on()) return hipMalloc(out, bytes);
  char *base = nullptr;
  const size_t padded = (bytes + 255) / 256 * 256;          // the rear band starts 256-byte aligned behind the payload's end
  hipError_t e = hipMalloc((void **)&base, padded + 2 * (size_t)MISIFT_GUARD_BYTES);
  if (e != hipSuccess) return e;
  if ((e = hipMemset(base, GUARD_BAND_BYTE, padded + 2 * (size_t)MISIFT_GUARD_BYTES)) != hipSuccess) return e;
  if ((e = hipMemset(base + MISIFT_GUARD_BYTES, GUARD_POISON_BYTE, bytes)) != hipSuccess) return e;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
  GuardRec r;
  r.base = base; r.bytes = bytes;
  snprintf(r.tag, sizeof(r.tag), "%s", tag ? tag : "?");
  std::lock_guard<std::mutex> lk(g_guard_mu);
  g_guard_map[base + MISIFT_GUARD_BYTES] = r;
  *out = base + MISIFT_GUARD_BYTES;
  return hipSuccess;
}
// bands of one guarded allocation: 0 = intact, 1 = damaged (the first damage of a process is described in g_guard_first), -1 = copy failed
static int g_guard_freed_damaged = 0, g_guard_freed_checked = 0;
static char g_guard_first[256];
static int guard_check_one(const GuardRec &r)
{
  const size_t padded = (r.bytes + 255) / 256 * 256;
  const size_t rear = padded - r.bytes + MISIFT_GUARD_BYTES;
  std::vector<unsigned char> host(MISIFT_GUARD_BYTES + rear);
  if (hipMemcpy(host.data(), r.base, MISIFT_GUARD_BYTES, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(host.data() + MISIFT_GUARD_BYTES, r.base + MISIFT_GUARD_BYTES + r.bytes, rear, hipMemcpyDeviceToHost) != hipSuccess)
    return -1;
  for (size_t i = 0; i < host.size(); i++)
    if (host[i] != GUARD_BAND_BYTE) {
      if (!g_guard_first[0]) {
        if (i < MISIFT_GUARD_BYTES)
          snprintf(g_guard_first, sizeof(g_guard_first), "guard band damaged: allocation '%s' (%zu bytes), %zu bytes IN FRONT of the payload",
                   r.tag, r.bytes, (size_t)MISIFT_GUARD_BYTES - i);
        else
          snprintf(g_guard_first, sizeof(g_guard_first), "guard band damaged: allocation '%s' (%zu bytes), %zu bytes BEHIND the payload's end",
                   r.tag, r.bytes, i - MISIFT_GUARD_BYTES);
      }
      return 1;
    }
  return 0;
}
hipError_t misift_dev_free(void *ptr)
{
  if (!ptr) return hipSuccess;
  {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    auto it = g_guard_map.find(ptr);
    if (it != g_guard_map.end()) {
      // a guarded buffer is verified when it goes, too: the caller's images / scratch arenas / record arrays usually live
      // for one call only and are gone by the time anyone asks misift_test_check_guards
      (void)hipDeviceSynchronize();
      g_guard_freed_checked++;
      if (guard_check_one(it->second) != 0) g_guard_freed_damaged++;
      char *base = it->second.base;
      g_guard_map.erase(it);
      return hipFree(base);
    }
  }
  return hipFree(ptr);
}
// Switch guard mode on / off for the allocations made FROM NOW ON (live allocations keep what they have).  Returns the old mode.
extern "C" int misift_test_set_guard(int on)
{
  const int old = guard_on() ? 1 : 0;
  g_guard_mode = on ? 1 : 0;
  return old;
}
// Verify the bands of every live guarded allocation (the whole device is synchronised first).  Returns the number of damaged
// allocations (misift_last_error() names the first: tag, size, band, offset of the first wrong byte), or a negative status;
// *allocations (optional) = live guarded allocations checked.  The payload between tail and rear band (the padding to 256
// bytes) counts as band.
extern "C" int misift_test_check_guards(int *allocations)
{
  if (hipDeviceSynchronize() != hipSuccess) { misift_set_error("misift_test_check_guards: hipDeviceSynchronize failed"); return -MISIFT_EHIP; }
  std::lock_guard<std::mutex> lk(g_guard_mu);
  int bad = g_guard_freed_damaged, n = g_guard_freed_checked;       // allocations freed since the last check were verified as they went
  g_guard_freed_damaged = 0; g_guard_freed_checked = 0;
  for (auto &kv : g_guard_map) {
    const int r = guard_check_one(kv.second);
    if (r < 0) { misift_set_error("misift_test_check_guards: copy of the bands of '%s' failed", kv.second.tag); return -MISIFT_EHIP; }
    n++;
    bad += r;
  }
  if (bad) misift_set_error("%s", g_guard_first);
  g_guard_first[0] = 0;
  if (allocations) *allocations = n;
  return bad;
}

extern "C" int misift_malloc(size_t bytes, void **out)
{
  ARG_CHECK(out != nullptr);
  *out = nullptr;
  if (bytes == 0) bytes = 16;
  hipError_t e = misift_dev_alloc(out, bytes, "misift_malloc");
  if (e != hipSuccess) {
    misift_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    return MISIFT_ENOMEM;
  }
  return MISIFT_OK;
}

extern "C" int misift_malloc_managed(size_t bytes, void **out)
{
  ARG_CHECK(out != nullptr);
  *out = nullptr;
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMallocManaged(out, bytes, hipMemAttachGlobal);
  if (e != hipSuccess) {
    misift_set_error("hipMallocManaged(%zu) failed: %s", bytes, hipGetErrorString(e));
    return MISIFT_ENOMEM;
  }
  return MISIFT_OK;
}

extern "C" int misift_free(void *ptr)
{
  if (ptr) HIP_TRY(misift_dev_free(ptr));
  return MISIFT_OK;
}

extern "C" int misift_memset(misift_ctx *ctx, void *ptr, int value, size_t bytes)
{
  ARG_CHECK(ctx && ptr);
  HIP_TRY(hipMemsetAsync(ptr, value, bytes, ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_copy_h2d(misift_ctx *ctx, void *dst, const void *src, size_t bytes)
{
  ARG_CHECK(ctx && dst && src);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_copy_d2h(misift_ctx *ctx, void *dst, const void *src, size_t bytes)
{
  ARG_CHECK(ctx && dst && src);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

static inline int ialign_up(int a, int b) { return (a % b != 0) ? (a - a % b + b) : a; }

extern "C" int misift_image_alloc(int width, int height, float **d_out, int *pitch_floats)
{
  ARG_CHECK(width > 0 && height > 0 && d_out && pitch_floats);
  const int p = ialign_up(width, 128);
  void *ptr = nullptr;
  int rc = misift_malloc(sizeof(float) * (size_t)p * height, &ptr);
  if (rc) return rc;
  *d_out = (float *)ptr;
  *pitch_floats = p;
  return MISIFT_OK;
}

extern "C" int misift_upload_2d(misift_ctx *ctx, float *d_dst, int dpitch, const float *h_src, int hpitch, int width,
                                int height)
{
  ARG_CHECK(ctx && d_dst && h_src && width > 0 && height > 0);
  HIP_TRY(hipMemcpy2DAsync(d_dst, sizeof(float) * (size_t)dpitch, h_src, sizeof(float) * (size_t)hpitch,
                           sizeof(float) * (size_t)width, height, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_download_2d(misift_ctx *ctx, float *h_dst, int hpitch, const float *d_src, int dpitch, int width,
                                  int height)
{
  ARG_CHECK(ctx && h_dst && d_src && width > 0 && height > 0);
  HIP_TRY(hipMemcpy2DAsync(h_dst, sizeof(float) * (size_t)hpitch, d_src, sizeof(float) * (size_t)dpitch,
                           sizeof(float) * (size_t)width, height, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_download_fields(misift_ctx *ctx, void *h_pts, const void *d_pts, int npts, int offset, int nfields)
{
  ARG_CHECK(ctx && h_pts && d_pts && npts >= 0 && offset >= 0 && nfields > 0 &&
            offset + 4 * nfields <= MISIFT_POINT_BYTES);
  if (npts == 0) return MISIFT_OK;
  HIP_TRY(hipMemcpy2DAsync((char *)h_pts + offset, MISIFT_POINT_BYTES, (const char *)d_pts + offset,
                           MISIFT_POINT_BYTES, 4 * (size_t)nfields, npts, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

// Reference sizing (cudaSiftH.cu:39-57): sums numOctaves+1 levels, kept for compatibility.
static void scratch_sizes(int width, int height, int num_octaves, int scale_up, size_t *size_img, size_t *size_tmp)
{
  const int nd = NUM_SCALES + 3;
  int w = width * (scale_up ? 2 : 1), h = height * (scale_up ? 2 : 1);
  int p = ialign_up(w, 128);
  size_t size = (size_t)h * p, sizeTmp = (size_t)nd * h * p;
  for (int i = 0; i < num_octaves; i++) {
    w /= 2;
    h /= 2;
    const int p2 = ialign_up(w, 128);
    size += (size_t)h * p2;
    sizeTmp += (size_t)nd * h * p2;
  }
  *size_img = size;
  *size_tmp = sizeTmp;
}

extern "C" size_t misift_scratch_floats(int width, int height, int num_octaves, int scale_up)
{
  size_t a, b;
  scratch_sizes(width, height, num_octaves, scale_up, &a, &b);
  size_t total = a + b;
  return (total + 4095) / 4096 * 4096;     // the reference rounds the arena to 4096-float rows (:58)
}

// -------------------------------------------------------------- host taps
// cudaSiftH.cu:408-418
static void lowpass_taps(float scale, float k[9])
{
  float kernelSum = 0.0f;
  const float ivar2 = 1.0f / (2.0f * scale * scale);
  for (int j = -4; j <= 4; j++) {
    k[j + 4] = (float)expf((float)(-(double)j * j * ivar2));
    kernelSum += k[j + 4];
  }
  for (int j = -4; j <= 4; j++) k[j + 4] /= kernelSum;
}

// cudaSiftH.cu:316-323
static void scaledown_taps(float variance, float k[5])
{
  float kernelSum = 0.0f;
  for (int j = 0; j < 5; j++) {
    k[j] = (float)expf((float)(-(double)(j - 2) * (j - 2) / 2.0 / variance));
    kernelSum += k[j];
  }
  for (int j = 0; j < 5; j++) k[j] /= kernelSum;
}

// cudaSiftH.cu:439-458
static void laplace_taps_rec(int numOctaves, float initBlur, float *kernel)
{
  if (numOctaves > 1) {
    const float totInitBlur = sqrtf(initBlur * initBlur + 0.5f * 0.5f) / 2.0f;
    laplace_taps_rec(numOctaves - 1, totInitBlur, kernel);
  }
  float scale = powf(2.0f, -1.0f / NUM_SCALES);
  const float diffScale = powf(2.0f, 1.0f / NUM_SCALES);
  for (int i = 0; i < NUM_SCALES + 3; i++) {
    float kernelSum = 0.0f;
    const float var = scale * scale - initBlur * initBlur;
    for (int j = 0; j <= 4; j++) {
      kernel[numOctaves * 12 * 16 + 16 * i + j] = (float)expf((float)(-(double)j * j / 2.0 / var));
      kernelSum += (j == 0 ? 1 : 2) * kernel[numOctaves * 12 * 16 + 16 * i + j];
    }
    for (int j = 0; j <= 4; j++) kernel[numOctaves * 12 * 16 + 16 * i + j] /= kernelSum;
    scale *= diffScale;
  }
}

extern "C" int misift_laplace_taps(int num_octaves, float *taps)
{
  ARG_CHECK(taps && num_octaves >= 1 && num_octaves <= MISIFT_MAX_OCTAVES);
  memset(taps, 0, sizeof(float) * 8 * 12 * 16);
  laplace_taps_rec(num_octaves, 0.0f, taps);
  return MISIFT_OK;
}

static LaplaceTaps octave_taps(const float *table, int octave)
{
  LaplaceTaps t;
  for (int s = 0; s < NUM_BLURS; s++)
    for (int j = 0; j < 5; j++) t.k[s][j] = table[octave * 12 * 16 + 16 * s + j];
  return t;
}

// ---------------------------------------------------------------- geometry
static StripGeom make_geom(misift_ctx *ctx, int w, int h, int pitch, int nframes, long long frame_stride,
                           int out_w, int out_rows, int out_lanes)
{
  StripGeom g;
  g.width = w; g.height = h; g.pitch = pitch;
  g.nframes = nframes; g.frame_stride = frame_stride;
  const int nquads = (out_w + 3) / 4;
  g.nstrips = (nquads + out_lanes - 1) / out_lanes;
  if (g.nstrips < 1) g.nstrips = 1;
  // aim for ~16 wavefronts per CU across the launch; segments between 8 and 128 rows
  const long long target = (long long)ctx->num_cus * ctx->strip_waves_per_cu;
  long long want = (target + (long long)nframes * g.nstrips - 1) / ((long long)nframes * g.nstrips);
  if (want < 1) want = 1;
  int seg = (int)((out_rows + want - 1) / want);
  if (nframes <= ctx->small_frames) {         // a frame or two: latency-bound, short (even) segments on every SIMD
    seg = (seg + 1) / 2 * 2;
    if (seg < ctx->strip_rows_small) seg = ctx->strip_rows_small;
  } else {
    seg = (seg + 7) / 8 * 8;
    if (seg < 8) seg = 8;
  }
  if (seg > 128) seg = 128;
  g.seg_rows = seg;
  g.nsegs = (out_rows + seg - 1) / seg;
  if (g.nsegs < 1) g.nsegs = 1;
  // bit 1: strip-fastest item order — the 4 wavefronts of a workgroup stream 4 KB contiguous per image row
  // (measured -20 % on lowpass vs segment-fastest: better HBM page locality); bit 0 would disable the XCD remap
  g.noremap = 2;
  return g;
}

// --------------------------------------------------------------- selftest
__global__ void selftest_kernel(float *out)
{
  const int lane = threadIdx.x;
  const float v = (float)(lane + 1);
  out[lane] = lane_from_left(v);          // expect lane      (0 for lane 0)
  out[64 + lane] = lane_from_right(v);    // expect lane + 2  (0 for lane 63)
}

int launch_selftest(misift_ctx *ctx)
{
  float *d = nullptr;
  float h[128];
  HIP_TRY(hipMalloc((void **)&d, sizeof(h)));
  hipLaunchKernelGGL(selftest_kernel, dim3(1), dim3(64), 0, ctx->stream, d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipFree(d));
  for (int l = 1; l < 64; l++)
    if (h[l] != (float)l) {
      misift_set_error("selftest: DPP wave_shr:1 lane %d got %g, expected %d", l, h[l], l);
      return MISIFT_EHIP;
    }
  for (int l = 0; l < 63; l++)
    if (h[64 + l] != (float)(l + 2)) {
      misift_set_error("selftest: DPP wave_shl:1 lane %d got %g, expected %d", l, h[64 + l], l + 2);
      return MISIFT_EHIP;
    }
  return MISIFT_OK;
}

// -------------------------------------------------------------- extraction
struct Level { int w, h, p; float *img; };   // img = frame-0 pointer of that pyramid level

// Arena layout of cudaSiftH.cu:104-107, :151-159, :179-184 inside one frame's arena: size_tmp floats of DoG space, then the
// pyramid levels, finest (num_octaves) first, each with rows padded to 128 floats.  off[o] = float offset of level o.
struct LevelDim { int w, h, p; long long off; };
static void pyramid_levels(int width, int height, int num_octaves, int scale_up, LevelDim *lv /* [num_octaves + 1] */)
{
  size_t size_img, size_tmp;
  scratch_sizes(width, height, num_octaves, scale_up, &size_img, &size_tmp);
  int w = width * (scale_up ? 2 : 1), h = height * (scale_up ? 2 : 1);
  long long off = (long long)size_tmp;
  for (int o = num_octaves; o >= 1; o--) {
    lv[o].w = w; lv[o].h = h; lv[o].p = ialign_up(w, 128); lv[o].off = off;
    off += (long long)h * lv[o].p;
    w /= 2; h /= 2;
  }
}

extern "C" int misift_test_pyramid_layout(int width, int height, int num_octaves, int scale_up, long long *offsets,
                                          int *widths, int *heights, int *pitches)
{
  ARG_CHECK(width >= 1 && height >= 1 && num_octaves >= 1 && num_octaves <= MISIFT_MAX_OCTAVES);
  ARG_CHECK(offsets && widths && heights && pitches);
  LevelDim lv[MISIFT_MAX_OCTAVES + 1];
  pyramid_levels(width, height, num_octaves, scale_up ? 1 : 0, lv);
  for (int o = num_octaves, i = 0; o >= 1; o--, i++) {
    offsets[i] = lv[o].off; widths[i] = lv[o].w; heights[i] = lv[o].h; pitches[i] = lv[o].p;
  }
  return MISIFT_OK;
}

// Test-only, host state only (no HIP call): the decomposition make_geom gives a streaming launch of this context — with
// its CU count and its knobs as they stand — as out = {nstrips, seg_rows, nsegs}.
extern "C" int misift_test_strip_geom(misift_ctx *ctx, int w, int h, int pitch, int nframes, int out_w, int out_rows,
                                      int out_lanes, int *out)
{
  ARG_CHECK(ctx && out && w >= 1 && h >= 1 && pitch >= w && nframes >= 1);
  ARG_CHECK(out_w >= 1 && out_rows >= 1 && out_lanes >= 1);
  const StripGeom g = make_geom(ctx, w, h, pitch, nframes, 0, out_w, out_rows, out_lanes);
  out[0] = g.nstrips; out[1] = g.seg_rows; out[2] = g.nsegs;
  return MISIFT_OK;
}

// Images under 16 x 16, or whose coarsest pyramid level is under 8 px: the reference runs them (levels shrink to a few
// pixels, every access clamped: cudaSiftH.cu:72-167) and so do we — on the dense per-level kernels, whose quad loads clamp
// at any width >= 1.  The merged-octave kernels (tiled prefilter, cone chain, strips sized for whole wavefronts) are
// built for images that fill at least a strip and never see such calls.  A level that integer division has shrunk to
// 0 pixels holds nothing and is skipped (CUDA itself refuses a zero-sized grid there).
// (options.reference_cap no longer sends a call here, r06: the fused path counts the true extrema of every 30 x 8 block in
//  refine_all and only a frame in which a block reaches a 33rd is redone on the dense kernels — the candidate-overflow
//  mechanism — where launch_refcap applies the cap in the reference's order.)
static bool dense_call(misift_ctx *ctx, int width, int height, int num_octaves)
{
  (void)ctx;
  return misift_tiny_call(width, height, num_octaves);
}
bool misift_tiny_call(int width, int height, int num_octaves)
{
  if (num_octaves < 1) return false;
  return width < 16 || height < 16 || (width >> (num_octaves - 1)) < 8 || (height >> (num_octaves - 1)) < 8;
}

// The level table of the merged-octave kernels for a call's pyramid (dims[o]: level o as pyramid_levels lays it out, off =
// float offset inside a frame's arena; SS = floats between the frames' arenas).  Returns the candidate slots one frame
// needs (the sum of the octaves' cand_cap).
static unsigned fill_pyramid_info(const misift_ctx *ctx, PyramidInfo *P, const LevelDim *dims, int num_octaves, int nframes,
                                  long long SS, float lowest_scale, int scale_up)
{
  P->noct = num_octaves; P->nframes = nframes; P->frame_stride = SS;
  P->fix_numpts = ctx->opt.fix_numpts ? 1 : 0;
  P->patch_reach = ctx->patch_reach;
  P->out_scale = scale_up ? 0.5f : 1.0f;             // RescalePositions (cudaSiftH.cu:130) folded into the record write
  unsigned off = 0;
  for (int o = 1; o <= num_octaves; o++) {
    OctaveInfo &L = P->o[o];
    L.w = dims[o].w; L.h = dims[o].h; L.p = dims[o].p;
    L.img_off = dims[o].off;
    L.subsampling = (float)(1 << (num_octaves - o));
    L.lowest_scale = lowest_scale / L.subsampling;
    size_t c = (size_t)L.w * L.h / 4;
    if (c < 16384) c = 16384;
    L.cand_cap = (unsigned)c;
    L.cand_off = off;
    off += L.cand_cap;
  }
  return off;
}

// The per-keypoint tail of the merged-octave sequence: every octave's detections wait in the staging area (d_det, their
// counts in CNT_DET + o) and the pyramid levels in the arena; this orders them, computes orientations and descriptors and
// writes the records in the reference's segment order.  Called by misift_extract_enqueue behind refine_all, and by
// misift_test_describe_detections on detections the caller supplies (allow_fuse = false: never the fused launch).
static int enqueue_keypoint_tail(misift_ctx *ctx, const float *d_scratch, const PyramidInfo &P, SiftPointD *pts, int max_pts,
                                 bool allow_fuse)
{
  int rc;
  // (a counting sort per (octave, frame) is one workgroup each: for a frame or two it is a dependent dispatch that buys
  //  nothing — the keypoints of one frame share the caches anyway)
  const bool binned = (ctx->bin_detections && P.nframes >= ctx->bin_min_frames) || ctx->opt.deterministic;
  ctx->cur_binned = binned ? 1 : 0;
  ctx->cur_balanced = 0;              // set by launch_bin_detections (its extra workgroup builds the block tables) or, without binning, by build_block_maps
  if (binned) {                       // spatial order for the per-keypoint kernels (L1/L2 reuse between neighbours);
    rc = launch_bin_detections(ctx, P, max_pts);      // deterministic mode: a total order
    if (rc) return rc;
  }
  // a frame or two: orientations and descriptors in one launch (the descriptor pass of a workgroup waits in the kernel for
  // the coarser octaves' orientations, whose duplicate counts decide where its records go)
  // (off by default: measured 12 us slower than the two launches)
  if (allow_fuse && ctx->fuse_orient && !binned && !ctx->pack_dst && P.nframes <= ctx->small_frames && ctx->tile_descr && !ctx->tile_orient &&
      !ctx->in_capture)
    return launch_orient_descr_fused(ctx, d_scratch, P, pts, max_pts);
  rc = launch_orient_all(ctx, d_scratch, P, pts, max_pts);
  if (rc) return rc;
  if (ctx->opt.deterministic) {       // second-orientation slots in keypoint order instead of atomic order
    rc = launch_renumber_dups(ctx, P, max_pts);
    if (rc) return rc;
  }
  if (ctx->pack_dst) {                // counts and offsets are known as soon as the orientations are: pack while writing
    rc = launch_export_counts_staged(ctx, P.nframes, P.noct, max_pts, ctx->pack_counts, ctx->pack_offsets);
    if (rc) return rc;
  }
  return launch_descr_all(ctx, d_scratch, P, pts, max_pts, ctx->pack_offsets, ctx->pack_dst);
}

// Enqueue the whole launch sequence of one batch on the context stream (no synchronisation).
// d_imgs: fp32 frames, or 8-bit frames when src_u8 (pitch / frame_stride in source elements).
int misift_extract_enqueue(misift_ctx *ctx, const void *d_imgs, int src_u8, int nframes, long long frame_stride,
                           int width, int height, int pitch, int num_octaves, float init_blur, float thresh,
                           float lowest_scale, int scale_up, float *d_scratch, SiftPointD *pts, int max_pts)
{
  RoctxRange range("misift_extract");
  ARG_CHECK(ctx && d_imgs && (pts || (ctx->pack_dst && ctx->opt.fused)));
  extra(ctx)->last_lane = nullptr;      // this batch runs on the context itself: its counters / stream are the results'
  extra(ctx)->last_done = nullptr;
  ARG_CHECK(nframes >= 1 && width >= 1 && height >= 1 && pitch >= width);
  ARG_CHECK(num_octaves >= 1 && num_octaves <= MISIFT_MAX_OCTAVES);       // before the shifts below
  const bool tiny = misift_tiny_call(width, height, num_octaves);
  // the entry points route tiny calls to the dense kernels (TinyScope)
  ARG_CHECK(!(tiny && ctx->opt.fused));
  ARG_CHECK(max_pts >= 1);
  ARG_CHECK(width * (scale_up ? 2 : 1) < 16384 && height * (scale_up ? 2 : 1) < 16384);
  HIP_TRY(hipSetDevice(ctx->device));
  // candidate list: pre-candidates of the fused scan (or true extrema of the unfused detect) of ONE
  // octave; sized from the image, not from max_pts (overflow is detected and handled by the callers)
  size_t cap = (size_t)width * height * (scale_up ? 4 : 1) / 4;
  if (cap < 65536) cap = 65536;
  int rc = misift_ensure_frames(ctx, nframes, cap);
  if (rc) return rc;
  const size_t S = misift_scratch_floats(width, height, num_octaves, scale_up);
  if (!d_scratch) {
    if (ctx->own_scratch_floats < S * nframes) {
      if (ctx->d_own_scratch) HIP_TRY(misift_dev_free(ctx->d_own_scratch));
      ctx->d_own_scratch = nullptr; ctx->own_scratch_floats = 0;
      HIP_TRY(misift_dev_alloc((void **)&ctx->d_own_scratch, sizeof(float) * S * nframes, "own_scratch"));
      ctx->own_scratch_floats = S * nframes;
    }
    d_scratch = ctx->d_own_scratch;
  }
  // (the frames' counter blocks are cleared by the prefilter kernel — the first kernel of every path below)
  ctx->exported = 0;

  // the tap tables depend on (num_octaves, init_blur) only: a few hundred expf / powf, i.e. microseconds of host time in
  // front of the first launch of EVERY call — cached per context (r04 single-call budget)
  CtxExtra *xt = extra(ctx);
  if (xt->taps_noct != num_octaves) {
    misift_laplace_taps(num_octaves, xt->taps_table);          // cudaSiftH.cu:109-111
    xt->taps_noct = num_octaves;
  }
  const float blur = init_blur > 0.001f ? init_blur : 0.001f;
  if (!(xt->k9_blur == blur)) {
    lowpass_taps(blur, xt->k9);
    xt->k9_blur = blur;
  }
  if (!xt->k5_done) {
    scaledown_taps(0.5f, xt->k5);
    xt->k5_done = true;
  }
  const float *table = xt->taps_table, *k9 = xt->k9, *k5 = xt->k5;

  // arena layout (per frame, frame stride S): pyramid_levels
  const int W = width * (scale_up ? 2 : 1), H = height * (scale_up ? 2 : 1);
  float *memoryTmp = d_scratch;
  std::vector<Level> lv(num_octaves + 1);
  {
    LevelDim dims[MISIFT_MAX_OCTAVES + 1];
    pyramid_levels(width, height, num_octaves, scale_up, dims);
    for (int o = num_octaves; o >= 1; o--) {
      lv[o].w = dims[o].w; lv[o].h = dims[o].h; lv[o].p = dims[o].p; lv[o].img = d_scratch + dims[o].off;
    }
  }
  const long long SS = (long long)S;
  // --- prefilter (cudaSiftH.cu:112 / :119-123); when the shape allows, the first ScaleDown of the pyramid is
  // produced by the same kernel (the prefiltered rows are decimated while still in registers)
  int first_down_done = 0;
  {
    const Level &L = lv[num_octaves];
    const void *pre_src = d_imgs;
    int pre_u8 = src_u8, pre_pitch = pitch, pre_frames = nframes;
    long long pre_stride = frame_stride;
    if (scale_up) {
      float *upImg = memoryTmp;
      // every frame's up-sampled copy borrows the DoG region of its own arena (cudaSiftH.cu:119-123)
      rc = launch_scaleup(ctx, d_imgs, src_u8, width, height, pitch, frame_stride, nframes, upImg, L.p, SS);
      if (rc) return rc;
      pre_src = upImg; pre_u8 = 0; pre_pitch = L.p; pre_frames = nframes; pre_stride = SS;
      lowest_scale *= 2.0f;
    }
    if (num_octaves >= 2 && ctx->opt.fused && ctx->lowpass_tile && nframes <= ctx->small_frames) {
      const Level &D = lv[num_octaves - 1];        // a frame or two: the LDS-tiled form (latency, not throughput)
      rc = launch_lowpass_down_tile(ctx, pre_src, pre_u8, W, H, pre_pitch, pre_stride, pre_frames, L.img, L.p, SS, k9, D.img,
                                    D.p, SS, k5, ctx->d_counters);
      if (rc) return rc;
      first_down_done = 1;
    } else if (num_octaves >= 2 && ctx->opt.fused) {
      const Level &D = lv[num_octaves - 1];
      StripGeom g = make_geom(ctx, W, H, pre_pitch, pre_frames, pre_stride, W, H, 60);
      rc = launch_lowpass_down(ctx, pre_src, pre_u8, g, L.img, L.p, SS, k9, D.img, D.p, SS, k5, &first_down_done,
                               ctx->d_counters);
      if (rc) return rc;
    }
    if (!first_down_done) {
      StripGeom g = make_geom(ctx, W, H, pre_pitch, pre_frames, pre_stride, W, H, 62);
      rc = launch_lowpass(ctx, pre_src, pre_u8, g, L.img, L.p, SS, k9, ctx->d_counters);
      if (rc) return rc;
    }
  }
  // --- merged-octave path: its level table is needed before the pyramid is built (split-tail mode below)
  PyramidInfo P;
  memset(&P, 0, sizeof(P));
  std::vector<LaplaceTaps> tapsv(num_octaves + 1);
  if (ctx->opt.fused) {
    LevelDim dims[MISIFT_MAX_OCTAVES + 1];
    for (int o = 1; o <= num_octaves; o++) {
      dims[o].w = lv[o].w; dims[o].h = lv[o].h; dims[o].p = lv[o].p; dims[o].off = (long long)(lv[o].img - d_scratch);
      tapsv[o] = octave_taps(table, o);
    }
    const unsigned off = fill_pyramid_info(ctx, &P, dims, num_octaves, nframes, SS, lowest_scale, scale_up);
    rc = misift_ensure_frames(ctx, nframes, off);
    if (rc) return rc;
    // the staging area is indexed with the CURRENT max_pts (kernels use it as the per-octave stride)
    rc = ensure_det(ctx, nframes, max_pts);
    if (rc) return rc;
  }
  // Split-tail mode: the two finest levels exist as soon as the fused prefilter has run, so their scan (most of
  // the scan work) starts at once on the context stream while the small ScaleDowns of the coarse levels and the
  // scan of those levels run beside it on a second, high-priority stream — their launch gaps and tails hide
  // under the big kernel.
  bool scanned = false;
  if (ctx->opt.fused && ctx->split_tail && nframes >= ctx->split_tail && !ctx->in_capture && first_down_done &&
      num_octaves >= 3 && ctx->stream2) {
    HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
    rc = launch_dog_scan_all(ctx, d_scratch, P, tapsv.data(), thresh, 0, 2);
    if (rc) return rc;
    hipStream_t saved = ctx->stream;
    ctx->stream = ctx->stream2;
    for (int o = num_octaves - 1; o >= 2 && !rc; o--) {
      const Level &src = lv[o], &dst = lv[o - 1];
      StripGeom g = make_geom(ctx, src.w, src.h, src.p, nframes, SS, dst.w, dst.h, 62);
      rc = launch_scaledown(ctx, src.img, g, dst.img, dst.p, SS, k5);
    }
    if (!rc) rc = launch_dog_scan_all(ctx, d_scratch, P, tapsv.data(), thresh, 2, num_octaves);
    ctx->stream = saved;
    if (rc) return rc;
    HIP_TRY(hipEventRecord(ctx->ev_join, ctx->stream2));
    HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    scanned = true;
  }
  // --- pyramid (ScaleDown chain of cudaSiftH.cu:153-160), finest to coarsest
  // Small batches (a single frame above all) are bound by the number of DEPENDENT dispatches, not by their work: up to
  // three levels per launch (scaledown_chain_kernel).  Batches keep one streamed launch per level.
  const bool chained = !scanned && !tiny && nframes <= ctx->chain_max_frames;
  // ... and when ONE chain covers every remaining level, it rides in the first workgroups of the scan launch
  ChainGeom embed;
  bool embedded = false;
  // (only where the host reads the counter blocks afterwards — the synchronous calls: that is where an expired wait is
  //  noticed and the call re-run, see read_counts)
  if (chained && ctx->opt.fused && ctx->chain_embed && ctx->want_export && first_down_done && num_octaves >= 3 &&
      num_octaves - 2 <= 3) {
    const int o = num_octaves - 1, nlev = o - 1;
    int dims[4][3];
    long long offs[4];
    for (int k = 0; k <= nlev; k++) {
      dims[k][0] = lv[o - k].w; dims[k][1] = lv[o - k].h; dims[k][2] = lv[o - k].p;
      offs[k] = (long long)(lv[o - k].img - d_scratch);
    }
    rc = make_chain_geom(&embed, SS, dims, offs, nlev, 4);
    if (rc) return rc;
    embedded = true;
  }
  for (int o = num_octaves; o >= 2 && !scanned && !embedded;) {
    if (o == num_octaves && first_down_done) { o--; continue; }
    if (chained) {
      const int nlev = (o - 1) < 3 ? (o - 1) : 3;
      int dims[4][3];
      long long offs[4];
      for (int k = 0; k <= nlev; k++) {
        dims[k][0] = lv[o - k].w; dims[k][1] = lv[o - k].h; dims[k][2] = lv[o - k].p;
        offs[k] = (long long)(lv[o - k].img - d_scratch);
      }
      rc = launch_scaledown_chain(ctx, d_scratch, SS, nframes, dims, offs, nlev, k5);
      if (rc) return rc;
      o -= nlev;
      continue;
    }
    const Level &src = lv[o], &dst = lv[o - 1];
    if (dst.w < 1 || dst.h < 1) break;                 // nothing left to decimate: this and every coarser level is empty
    StripGeom g = make_geom(ctx, src.w, src.h, src.p, nframes, SS, dst.w, dst.h, 62);
    rc = launch_scaledown(ctx, src.img, g, dst.img, dst.p, SS, k5);
    if (rc) return rc;
    o--;
  }
  if (ctx->opt.fused) {
    // scan / refine / orient / descr each run ONCE over all pyramid levels; the final array is laid out in the
    // reference's segment order by descr_all_kernel
    if (!scanned) {
      rc = launch_dog_scan_all(ctx, d_scratch, P, tapsv.data(), thresh, 0, num_octaves, embedded ? &embed : nullptr, k5);
      if (rc) return rc;
    }
    rc = launch_refine_all(ctx, d_scratch, P, tapsv.data(), thresh, 10.0f, 1.0f / NUM_SCALES, max_pts);
    if (rc) return rc;
    return enqueue_keypoint_tail(ctx, d_scratch, P, pts, max_pts, true);
  }
  // --- octaves, coarsest first (cudaSiftH.cu:161 after the recursion)
  for (int o = 1; o <= num_octaves; o++) {
    const Level &L = lv[o];
    if (L.w < 1 || L.h < 1) continue;                  // an empty level: no pixels, no points (counters stay where they are)
    const float subsampling = (float)(1 << (num_octaves - o));
    const LaplaceTaps taps = octave_taps(table, o);
    {
      StripGeom g = make_geom(ctx, L.w, L.h, L.p, nframes, SS, L.w, L.h, 62);
      rc = launch_laplace(ctx, L.img, g, memoryTmp, SS, taps);
      if (rc) return rc;
      rc = launch_detect(ctx, memoryTmp, g, SS, thresh, o);
      if (rc) return rc;
      if (ctx->opt.reference_cap) {
        rc = launch_refcap(ctx, L.w, L.h, nframes, o);
        if (rc) return rc;
      }
      rc = launch_refine(ctx, memoryTmp, SS, nullptr, 0, nullptr, L.w, L.h, L.p, nframes, thresh, 10.0f,
                         1.0f / NUM_SCALES, lowest_scale / subsampling, subsampling, o, pts, max_pts);
      if (rc) return rc;
    }
    rc = launch_orient(ctx, L.img, SS, L.w, L.h, L.p, nframes, o, pts, max_pts);
    if (rc) return rc;
    rc = launch_descr(ctx, L.img, SS, L.w, L.h, L.p, nframes, subsampling, o, pts, max_pts);
    if (rc) return rc;
  }
  if (ctx->opt.deterministic) {                     // dense path: order fixed after the fact, segment by segment
    rc = launch_sort_segments(ctx, pts, max_pts, nframes, num_octaves);
    if (rc) return rc;
  }
  if (scale_up) return launch_rescale_batch(ctx, pts, max_pts, nframes, num_octaves, 0.5f);      // cudaSiftH.cu:130
  return MISIFT_OK;
}

// Wait until a kernel of the context stream has stored `seq` into a word of pinned host memory: poll it (a few hundred
// ns after the store) instead of a blocking copy + hipStreamSynchronize.  The records themselves are complete for
// every later operation on the context's stream; a consumer on ANOTHER stream or device calls misift_ctx_sync first
// (include/misift.h).  MISIFT_HOST_SPIN=0: plain hipStreamSynchronize.
static int wait_host_flag(misift_ctx *ctx, unsigned *word, unsigned seq)
{
  volatile unsigned *flag = word;
  bool seen = false;
  if (ctx->host_spin) {
    for (unsigned spins = 0; !seen; spins++) {
      seen = *flag == seq;
#if defined(__x86_64__) || defined(__i386__)
      if (!seen) __builtin_ia32_pause();                   // a polite spin: the sibling hyper-thread keeps its issue slots
#endif
      if (!seen && (spins & 0x3fff) == 0x3fff) {           // every ~16 k polls: is the stream still alive?
        const hipError_t q = hipStreamQuery(ctx->stream);
        if (q == hipSuccess) { seen = *flag == seq; break; }
        if (q != hipErrorNotReady) HIP_TRY(q);
      }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    // keep the runtime's bookkeeping of finished commands bounded
    if ((seq & 63u) == 0) HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  if (!seen) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (*flag != seq) {
      misift_set_error("the kernel's completion flag did not arrive (flag %u, expected %u)", *flag, seq);
      return MISIFT_EHIP;
    }
  }
  return MISIFT_OK;
}

#define MISIFT_RETRY_CHAIN 1000      // internal to this file: never returned to a caller
#define MISIFT_RETRY_FUSE 1001
static int read_counts(misift_ctx *ctx, int nframes, int num_octaves, int max_pts, int *num_pts_out,
                       bool *cand_overflow)
{
  if (ctx->exported) {
    // the last kernel of the call has written the counter blocks into h_counters and stores export_seq behind them
    int rc = wait_host_flag(ctx, ctx->h_counters + (size_t)nframes * CNT_STRIDE, ctx->export_seq);
    if (rc) return rc;
    if (ctx->pending_big.valid) {
      // a folded single call (launch_descr_all): descr_all exported the counters; descr_big runs only if some keypoint was
      // deferred to it — next to never — and exports them again
      bool any = false;
      for (int f = 0; f < nframes; f++) any = any || ctx->h_counters[(size_t)f * CNT_STRIDE + CNT_BIG] != 0;
      if (!any) ctx->pending_big.valid = 0;
      else {
        rc = launch_descr_big_pending(ctx);
        if (!rc) rc = wait_host_flag(ctx, ctx->h_counters + (size_t)nframes * CNT_STRIDE, ctx->export_seq);
        if (rc) return rc;
      }
    }
  } else {
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(unsigned) * CNT_STRIDE * (size_t)nframes,
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  if (ctx->h_counters[CNT_CHAINTMO]) return MISIFT_RETRY_CHAIN;      // dog_scan_all_kernel: the bounded in-launch wait expired
  if (ctx->h_counters[CNT_FUSETMO]) return MISIFT_RETRY_FUSE;        // orient_descr_fused_kernel: likewise
  const int slot = 2 * num_octaves + (ctx->opt.fix_numpts ? 1 : 0);
  for (int f = 0; f < nframes; f++) {
    const unsigned c = ctx->h_counters[(size_t)f * CNT_STRIDE + slot];
    num_pts_out[f] = (int)(c < (unsigned)max_pts ? c : (unsigned)max_pts);     // cudaSiftH.cu:116
    if (ctx->h_counters[(size_t)f * CNT_STRIDE + CNT_CANDOVF]) *cand_overflow = true;
  }
  return MISIFT_OK;
}

// Run the launch sequence and read the counts back.  If a candidate list overflowed in the fused
// path (possible only for extreme thresh/contrast), redo the batch with the dense unfused kernels,
// whose list holds true 3x3x3 extrema only; an overflow there is reported as an error, never dropped
// silently (the reference silently caps at 32 candidates per 30x8 tile, cudaSiftD.cu:1371).
// Enqueue through a captured hipGraph when this exact call was seen before: the first call runs normally (and
// allocates whatever the context needs), the second is captured while it is enqueued, later ones are one
// hipGraphLaunch instead of ~10 launches.  Returns 1 if the work was queued here, 0 if the caller must enqueue it
// the ordinary way (graphs disabled, profiling on, unsuitable call, or any capture problem — which turns graphs off).
static int enqueue_via_graph(misift_ctx *ctx, const CallKey &key, const void *d_imgs, long long frame_stride,
                             float *d_scratch, SiftPointD *pts)
{
  CtxExtra *x = extra(ctx);
  if (!x->graph_mode || ctx->profile || !d_scratch || key.scale_up || !key.fused) return 0;
  if (x->have_graph && x->graph_key == key) {
    if (hipEventRecord(x->gev_in, ctx->stream) != hipSuccess || hipStreamWaitEvent(x->gstream, x->gev_in, 0) != hipSuccess ||
        hipGraphLaunch(x->gexec, x->gstream) != hipSuccess || hipEventRecord(x->gev_out, x->gstream) != hipSuccess ||
        hipStreamWaitEvent(ctx->stream, x->gev_out, 0) != hipSuccess) {
      (void)hipGetLastError();
      x->graph_mode = 0;
      return 0;
    }
    return 1;
  }
  const bool repeat = x->have_last && x->last_key == key;
  x->last_key = key;
  x->have_last = true;
  if (!repeat) return 0;
  // second identical call: capture it
  if (!x->gstream) {
    if (hipStreamCreateWithFlags(&x->gstream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&x->gev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x->gev_out, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      x->graph_mode = 0;
      return 0;
    }
  }
  if (x->have_graph) { hipGraphExecDestroy(x->gexec); x->gexec = nullptr; x->have_graph = false; }
  hipStream_t saved = ctx->stream;
  hipGraph_t graph = nullptr;
  if (hipStreamBeginCapture(x->gstream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    x->graph_mode = 0;
    return 0;
  }
  ctx->stream = x->gstream;
  ctx->in_capture = 1;
  const int rc = misift_extract_enqueue(ctx, d_imgs, key.src_u8, key.nframes, frame_stride, key.width, key.height,
                                        key.pitch, key.num_octaves, key.init_blur, key.thresh, key.lowest_scale, 0,
                                        d_scratch, pts, key.max_pts);
  ctx->stream = saved;
  ctx->in_capture = 0;
  const hipError_t e = hipStreamEndCapture(x->gstream, &graph);
  if (rc || e != hipSuccess || !graph || hipGraphInstantiate(&x->gexec, graph, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    if (graph) hipGraphDestroy(graph);
    x->gexec = nullptr;
    x->graph_mode = 0;                 // never try again on this context; the caller enqueues the ordinary way
    return 0;
  }
  hipGraphDestroy(graph);
  x->graph_key = key;
  x->have_graph = true;
  return enqueue_via_graph(ctx, key, d_imgs, frame_stride, d_scratch, pts);      // replay what was just captured
}

// The asynchronous entry points run a tiny call on the dense kernels as well (misift_tiny_call).
struct TinyScope {
  misift_ctx *ctx;
  int saved;
  TinyScope(misift_ctx *c, int w, int h, int noct) : ctx(c), saved(c ? c->opt.fused : 0)
  {
    if (ctx && dense_call(ctx, w, h, noct)) ctx->opt.fused = 0;
  }
  ~TinyScope() { if (ctx) ctx->opt.fused = saved; }
};

int misift_extract_sync(misift_ctx *ctx, const void *d_imgs, int src_u8, int nframes, long long frame_stride, int width,
                        int height, int pitch, int num_octaves, float init_blur, float thresh, float lowest_scale,
                        int scale_up, float *d_scratch, SiftPointD *pts, int max_pts, int *num_pts_out)
{
  ARG_CHECK(ctx != nullptr && num_pts_out != nullptr);
  // the option is restored on EVERY way out (incl. the HIP_TRY returns below) by a scope guard, not by hand
  struct FusedGuard {
    misift_ctx *c; int saved;
    ~FusedGuard() { c->opt.fused = saved; }
  } fused_guard{ctx, ctx->opt.fused};
  const int fused_saved = fused_guard.saved;
  if (dense_call(ctx, width, height, num_octaves)) ctx->opt.fused = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    int rc = MISIFT_OK;
    int queued = 0;
    if (attempt == 0 && ctx && d_imgs && pts) {
      CallKey key;
      memset(&key, 0, sizeof(key));
      key.imgs = d_imgs; key.scratch = d_scratch; key.pts = pts;
      key.src_u8 = src_u8; key.nframes = nframes; key.width = width; key.height = height; key.pitch = pitch;
      key.num_octaves = num_octaves; key.scale_up = scale_up; key.max_pts = max_pts; key.fused = ctx->opt.fused;
      key.texfrac = ctx->opt.texfrac_bits; key.fixnum = ctx->opt.fix_numpts; key.determ = ctx->opt.deterministic; key.refcap = ctx->opt.reference_cap; key.alloc_gen = ctx->alloc_gen;
      key.frame_stride = frame_stride; key.init_blur = init_blur; key.thresh = thresh; key.lowest_scale = lowest_scale;
      queued = enqueue_via_graph(ctx, key, d_imgs, frame_stride, d_scratch, pts);
    }
    if (!queued) {
      ctx->want_export = 1;              // the last kernel hands the counters to the host (paths that cannot leave it 0)
      rc = misift_extract_enqueue(ctx, d_imgs, src_u8, nframes, frame_stride, width, height, pitch, num_octaves,
                                  init_blur, thresh, lowest_scale, scale_up, d_scratch, pts, max_pts);
      ctx->want_export = 0;
    } else {
      ctx->exported = 0;                 // a replayed graph carries no fresh sequence number
    }
    bool ovf = false;
    if (!rc) rc = read_counts(ctx, nframes, num_octaves, max_pts, num_pts_out, &ovf);
    if (rc == MISIFT_RETRY_CHAIN && ctx->chain_embed) {
      // Some workgroup's bounded wait for the ScaleDown chain inside the scan launch expired: its items were skipped, the
      // records are incomplete.  Never again on this context: the chain becomes a launch of its own (one dependent
      // dispatch, ~5 us per call), and this call is redone that way.
      if (!ctx->opt.quiet)
        fprintf(stderr, "misift: the in-launch wait for the ScaleDown chain expired (workgroups were not dispatched in index "
                        "order?); this context now launches the chain separately\n");
      ctx->chain_embed = 0;
      ctx->chain_fallbacks++;
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      attempt--;
      continue;
    }
    if (rc == MISIFT_RETRY_FUSE && ctx->fuse_orient) {
      // Some workgroup of the fused orientation + descriptor launch gave up waiting for the coarser octaves' orientations and
      // skipped its descriptors.  Never again on this context: two launches, and this call is redone that way.
      if (!ctx->opt.quiet)
        fprintf(stderr, "misift: the in-launch wait of the fused orientation + descriptor kernel expired; this context now "
                        "launches the two kernels separately\n");
      ctx->fuse_orient = 0;
      ctx->fuse_fallbacks++;
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      attempt--;
      continue;
    }
    if (rc == MISIFT_RETRY_CHAIN || rc == MISIFT_RETRY_FUSE) rc = MISIFT_EHIP;
    if (rc) { ctx->opt.fused = fused_saved; return rc; }
    if (!ovf) break;
    if (ctx->opt.fused && attempt == 0) {
      // Exact re-run with the dense kernels — of the frames whose candidate list overflowed ONLY (r02 redid the whole
      // batch at 0.3x the fused rate for one bad frame).  Every run of consecutive overflowed frames is one sub-call on
      // its own slices of the inputs, the scratch arena and the output; its counters are merged into the batch's.
      std::vector<unsigned> merged(ctx->h_counters, ctx->h_counters + (size_t)CNT_STRIDE * nframes);
      const size_t S = misift_scratch_floats(width, height, num_octaves, scale_up);
      const size_t esz = src_u8 ? 1 : sizeof(float);
      ctx->opt.fused = 0;
      bool ovf2 = false;
      for (int f0 = 0; f0 < nframes && !rc;) {
        if (!merged[(size_t)f0 * CNT_STRIDE + CNT_CANDOVF]) { f0++; continue; }
        int f1 = f0 + 1;
        while (f1 < nframes && merged[(size_t)f1 * CNT_STRIDE + CNT_CANDOVF]) f1++;
        const int nr = f1 - f0;
        rc = misift_extract_enqueue(ctx, (const char *)d_imgs + (size_t)f0 * frame_stride * esz, src_u8, nr, frame_stride, width,
                                    height, pitch, num_octaves, init_blur, thresh, lowest_scale, scale_up,
                                    d_scratch ? d_scratch + (size_t)f0 * S : nullptr, pts + (size_t)f0 * max_pts, max_pts);
        if (!rc) rc = read_counts(ctx, nr, num_octaves, max_pts, num_pts_out + f0, &ovf2);
        if (!rc) memcpy(&merged[(size_t)f0 * CNT_STRIDE], ctx->h_counters, sizeof(unsigned) * CNT_STRIDE * (size_t)nr);
        f0 = f1;
      }
      ctx->opt.fused = fused_saved;
      if (rc) return rc;
      if (ovf2) {
        misift_set_error("candidate list overflow: more than %zu scale-space extrema in one octave of one frame "
                         "(raise thresh)", ctx->cand_cap);
        return MISIFT_ENOMEM;
      }
      // the batch's counters (misift_get_counters) are the merged ones
      memcpy(ctx->h_counters, merged.data(), sizeof(unsigned) * merged.size());
      HIP_TRY(hipMemcpyAsync(ctx->d_counters, ctx->h_counters, sizeof(unsigned) * merged.size(), hipMemcpyHostToDevice,
                             ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      return MISIFT_OK;
    }
    ctx->opt.fused = fused_saved;
    misift_set_error("candidate list overflow: more than %zu scale-space extrema in one octave of one frame "
                     "(raise thresh)", ctx->cand_cap);
    return MISIFT_ENOMEM;
  }
  ctx->opt.fused = fused_saved;
  return MISIFT_OK;
}

// Test-only (include/misift.h): the per-keypoint tail of the merged-octave sequence on detections and pyramid levels the
// caller supplies.  Everything the tail reads is set up as misift_extract_enqueue sets it up — arena layout, level table,
// candidate buffer (descr_big's list lives there), staging area, counter blocks — and the counters come back through
// read_counts, so a call of a frame or two runs the folded shape with its on-demand descr_big launch.
extern "C" int misift_test_describe_detections(misift_ctx *ctx, int nframes, int width, int height, int num_octaves,
                                               int scale_up, const float *const *levels, const float *dets,
                                               const int *det_counts, void *d_pts, int max_pts, int *num_pts)
{
  ARG_CHECK(ctx && levels && det_counts && d_pts && num_pts);
  ARG_CHECK(nframes >= 1 && width >= 1 && height >= 1 && max_pts >= 1);
  ARG_CHECK(num_octaves >= 1 && num_octaves <= MISIFT_MAX_OCTAVES);
  ARG_CHECK(width < 16384 && height < 16384);
  LevelDim dims[MISIFT_MAX_OCTAVES + 1];
  pyramid_levels(width, height, num_octaves, 0, dims);
  ARG_CHECK(dims[1].w >= 1 && dims[1].h >= 1);                  // the coarsest level holds a pixel, hence all do
  long long total = 0;
  for (int k = 0; k < nframes * num_octaves; k++) {
    ARG_CHECK(levels[k] != nullptr && det_counts[k] >= 0);
    total += det_counts[k];
  }
  ARG_CHECK(total == 0 || dets != nullptr);
  HIP_TRY(hipSetDevice(ctx->device));
  extra(ctx)->last_lane = nullptr;      // this call runs on the context itself, like misift_extract_enqueue
  extra(ctx)->last_done = nullptr;
  size_t cap = (size_t)width * height / 4;
  if (cap < 65536) cap = 65536;
  int rc = misift_ensure_frames(ctx, nframes, cap);
  if (rc) return rc;
  const size_t S = misift_scratch_floats(width, height, num_octaves, 0);
  if (ctx->own_scratch_floats < S * nframes) {
    if (ctx->d_own_scratch) HIP_TRY(misift_dev_free(ctx->d_own_scratch));
    ctx->d_own_scratch = nullptr; ctx->own_scratch_floats = 0;
    HIP_TRY(misift_dev_alloc((void **)&ctx->d_own_scratch, sizeof(float) * S * nframes, "own_scratch"));
    ctx->own_scratch_floats = S * nframes;
  }
  float *d_scratch = ctx->d_own_scratch;
  ctx->exported = 0;
  PyramidInfo P;
  memset(&P, 0, sizeof(P));
  const unsigned off = fill_pyramid_info(ctx, &P, dims, num_octaves, nframes, (long long)S, 0.0f, scale_up);
  rc = misift_ensure_frames(ctx, nframes, off);
  if (rc) return rc;
  rc = ensure_det(ctx, nframes, max_pts);
  if (rc) return rc;
  // the counter blocks as the prefilter leaves them (all zero, the spare blocks behind the last frame's included), then
  // what refine_all adds: the octaves' detection counts (uncapped) and the detections that found no room
  std::vector<unsigned> counters((size_t)CNT_STRIDE * ((size_t)nframes + CNT_SPARE_BLOCKS), 0u);
  std::vector<Detection> staged;
  const float *src = dets;
  for (int f = 0; f < nframes; f++)
    for (int o = 1; o <= num_octaves; o++) {
      const int k = f * num_octaves + (o - 1), n = det_counts[k], kept = n < max_pts ? n : max_pts;
      HIP_TRY(hipMemcpy2DAsync(d_scratch + (size_t)f * S + dims[o].off, sizeof(float) * (size_t)dims[o].p, levels[k],
                               sizeof(float) * (size_t)dims[o].w, sizeof(float) * (size_t)dims[o].w, dims[o].h,
                               hipMemcpyHostToDevice, ctx->stream));
      counters[(size_t)f * CNT_STRIDE + CNT_DET + o] = (unsigned)n;
      counters[(size_t)f * CNT_STRIDE + CNT_PTOVF] += (unsigned)(n - kept);
      staged.resize((size_t)kept);
      for (int i = 0; i < kept; i++) {
        const float *d = src + 5 * (size_t)i;
        staged[i] = Detection{d[0], d[1], d[2], d[3], d[4], 0.0f, 0.0f, -1};
      }
      src += 5 * (size_t)n;
      if (kept) {
        HIP_TRY(hipMemcpyAsync(ctx->d_det + ((size_t)f * MISIFT_MAX_OCTAVES + (o - 1)) * max_pts, staged.data(),
                               sizeof(Detection) * (size_t)kept, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));            // `staged` is reused for the next octave
      }
    }
  HIP_TRY(hipMemcpyAsync(ctx->d_counters, counters.data(), sizeof(unsigned) * counters.size(), hipMemcpyHostToDevice,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->want_export = 1;
  rc = enqueue_keypoint_tail(ctx, d_scratch, P, (SiftPointD *)d_pts, max_pts, false);
  ctx->want_export = 0;
  bool ovf = false;
  if (!rc) rc = read_counts(ctx, nframes, num_octaves, max_pts, num_pts, &ovf);
  if (rc == MISIFT_RETRY_CHAIN || rc == MISIFT_RETRY_FUSE) rc = MISIFT_EHIP;       // (neither kernel runs here)
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

// Test-only (include/misift.h): the detector of the merged-octave sequence — dog_scan_all, then refine_all — on pyramid
// levels the caller supplies.  Arena, level table, candidate / staging / counter buffers and the kernels' arguments are
// those of misift_extract_enqueue; the scan never carries the embedded ScaleDown chain (chain = NULL), and its two-range
// form is issued on the context's one stream.
extern "C" int misift_test_detect_levels(misift_ctx *ctx, int nframes, int width, int height, int num_octaves, float thresh,
                                         float lowest_scale, int scale_up, const float *const *levels, int max_pts,
                                         int two_ranges, unsigned int *cand, int cand_slots, int *cand_counts, float *dets,
                                         int *det_counts, unsigned int *counters, int *scan_geom)
{
  ARG_CHECK(ctx && levels && cand && cand_counts && dets && det_counts && counters && scan_geom);
  ARG_CHECK(nframes >= 1 && width >= 1 && height >= 1 && max_pts >= 1);
  ARG_CHECK(num_octaves >= 1 && num_octaves <= MISIFT_MAX_OCTAVES);
  ARG_CHECK(width < 16384 && height < 16384);
  ARG_CHECK(!misift_tiny_call(width, height, num_octaves));     // the entry points never send such a call to these kernels
  ARG_CHECK(two_ranges == 0 || (two_ranges == 1 && num_octaves >= 3));
  LevelDim dims[MISIFT_MAX_OCTAVES + 1];
  pyramid_levels(width, height, num_octaves, 0, dims);
  for (int k = 0; k < nframes * num_octaves; k++) ARG_CHECK(levels[k] != nullptr);
  PyramidInfo P;
  memset(&P, 0, sizeof(P));
  const size_t S = misift_scratch_floats(width, height, num_octaves, 0);
  if (scale_up) lowest_scale *= 2.0f;                           // as misift_extract_enqueue (cudaSiftH.cu:119-123)
  const unsigned off = fill_pyramid_info(ctx, &P, dims, num_octaves, nframes, (long long)S, lowest_scale, scale_up);
  for (int o = 1; o <= num_octaves; o++) ARG_CHECK((unsigned)cand_slots >= P.o[o].cand_cap);
  HIP_TRY(hipSetDevice(ctx->device));
  extra(ctx)->last_lane = nullptr;      // this call runs on the context itself, like misift_extract_enqueue
  extra(ctx)->last_done = nullptr;
  size_t cap = (size_t)width * height / 4;
  if (cap < 65536) cap = 65536;
  int rc = misift_ensure_frames(ctx, nframes, cap);
  if (rc) return rc;
  if (ctx->own_scratch_floats < S * nframes) {
    if (ctx->d_own_scratch) HIP_TRY(misift_dev_free(ctx->d_own_scratch));
    ctx->d_own_scratch = nullptr; ctx->own_scratch_floats = 0;
    HIP_TRY(misift_dev_alloc((void **)&ctx->d_own_scratch, sizeof(float) * S * nframes, "own_scratch"));
    ctx->own_scratch_floats = S * nframes;
  }
  float *d_scratch = ctx->d_own_scratch;
  ctx->exported = 0;
  rc = misift_ensure_frames(ctx, nframes, off);
  if (rc) return rc;
  rc = ensure_det(ctx, nframes, max_pts);
  if (rc) return rc;
  CtxExtra *xt = extra(ctx);
  if (xt->taps_noct != num_octaves) {
    misift_laplace_taps(num_octaves, xt->taps_table);
    xt->taps_noct = num_octaves;
  }
  std::vector<LaplaceTaps> tapsv(num_octaves + 1);
  for (int o = 1; o <= num_octaves; o++) tapsv[o] = octave_taps(xt->taps_table, o);
  for (int f = 0; f < nframes; f++)
    for (int o = 1; o <= num_octaves; o++)
      HIP_TRY(hipMemcpy2DAsync(d_scratch + (size_t)f * S + dims[o].off, sizeof(float) * (size_t)dims[o].p,
                               levels[f * num_octaves + (o - 1)], sizeof(float) * (size_t)dims[o].w,
                               sizeof(float) * (size_t)dims[o].w, dims[o].h, hipMemcpyHostToDevice, ctx->stream));
  // the counter blocks as the prefilter leaves them: all zero, the spare blocks behind the last frame's included
  HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned) * CNT_STRIDE * ((size_t)nframes + CNT_SPARE_BLOCKS), ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));                   // (the levels are pageable host memory)
  int geom[2 * MISIFT_MAX_OCTAVES];
  if (two_ranges) {                                             // split-tail mode's two launches, here on one stream
    rc = launch_dog_scan_all(ctx, d_scratch, P, tapsv.data(), thresh, 0, 2, nullptr, nullptr, geom);
    if (!rc) rc = launch_dog_scan_all(ctx, d_scratch, P, tapsv.data(), thresh, 2, num_octaves, nullptr, nullptr, geom + 4);
  } else {
    rc = launch_dog_scan_all(ctx, d_scratch, P, tapsv.data(), thresh, 0, num_octaves, nullptr, nullptr, geom);
  }
  if (!rc) rc = launch_refine_all(ctx, d_scratch, P, tapsv.data(), thresh, 10.0f, 1.0f / NUM_SCALES, max_pts);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(counters, ctx->d_counters, sizeof(unsigned) * CNT_STRIDE * (size_t)nframes, hipMemcpyDeviceToHost,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (int lev = 0; lev < num_octaves; lev++) {                 // geom: finest level first; scan_geom: by octave
    scan_geom[2 * (num_octaves - lev - 1)] = geom[2 * lev];
    scan_geom[2 * (num_octaves - lev - 1) + 1] = geom[2 * lev + 1];
  }
  std::vector<Detection> staged;
  for (int f = 0; f < nframes; f++)
    for (int o = 1; o <= num_octaves; o++) {
      const int k = f * num_octaves + (o - 1);
      const unsigned *cnt = counters + (size_t)f * CNT_STRIDE;
      const unsigned nc = cnt[CNT_CAND + o] < P.o[o].cand_cap ? cnt[CNT_CAND + o] : P.o[o].cand_cap;
      const unsigned nd = cnt[CNT_DET + o] < (unsigned)max_pts ? cnt[CNT_DET + o] : (unsigned)max_pts;
      cand_counts[k] = (int)nc;
      det_counts[k] = (int)nd;
      if (nc)
        HIP_TRY(hipMemcpyAsync(cand + (size_t)k * cand_slots, ctx->d_cand + (size_t)f * off + P.o[o].cand_off,
                               sizeof(unsigned) * nc, hipMemcpyDeviceToHost, ctx->stream));
      staged.resize(nd);
      if (nd)
        HIP_TRY(hipMemcpyAsync(staged.data(), ctx->d_det + ((size_t)f * MISIFT_MAX_OCTAVES + (o - 1)) * max_pts,
                               sizeof(Detection) * nd, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));               // `staged` is reused for the next octave
      float *out = dets + 5 * (size_t)k * max_pts;
      for (unsigned i = 0; i < nd; i++) {
        const Detection &d = staged[i];
        out[5 * i + 0] = d.xpos; out[5 * i + 1] = d.ypos; out[5 * i + 2] = d.scale;
        out[5 * i + 3] = d.sharpness; out[5 * i + 4] = d.edgeness;
      }
    }
  return resolve_profile(ctx);
}

extern "C" int misift_extract(misift_ctx *ctx, const float *d_img, int width, int height, int pitch, int num_octaves,
                              float init_blur, float thresh, float lowest_scale, int scale_up, float *d_scratch,
                              void *d_pts, int max_pts, int *num_pts_out)
{
  ARG_CHECK(num_pts_out != nullptr);
  int rc = misift_extract_sync(ctx, d_img, 0, 1, 0, width, height, pitch, num_octaves, init_blur, thresh, lowest_scale,
                        scale_up, d_scratch, (SiftPointD *)d_pts, max_pts, num_pts_out);
  if (rc) return rc;
  return resolve_profile(ctx);                       // RescalePositions (cudaSiftH.cu:130) is part of the launch sequence
}

extern "C" int misift_extract_batch(misift_ctx *ctx, const float *d_imgs, int nframes, size_t frame_stride, int width,
                                    int height, int pitch, int num_octaves, float init_blur, float thresh,
                                    float lowest_scale, float *d_scratch, void *d_pts, int max_pts,
                                    int *num_pts_out)
{
  ARG_CHECK(num_pts_out != nullptr);
  int rc = misift_extract_sync(ctx, d_imgs, 0, nframes, (long long)frame_stride, width, height, pitch, num_octaves,
                        init_blur, thresh, lowest_scale, 0, d_scratch, (SiftPointD *)d_pts, max_pts, num_pts_out);
  if (rc) return rc;
  return resolve_profile(ctx);
}

extern "C" int misift_extract_batch_ex(misift_ctx *ctx, const void *d_imgs, int src_u8, int nframes, size_t frame_stride,
                                       int width, int height, int pitch, int num_octaves, float init_blur, float thresh,
                                       float lowest_scale, int scale_up, float *d_scratch, void *d_pts, int max_pts,
                                       int *num_pts_out)
{
  ARG_CHECK(num_pts_out != nullptr);
  int rc = misift_extract_sync(ctx, d_imgs, src_u8 ? 1 : 0, nframes, (long long)frame_stride, width, height, pitch,
                               num_octaves, init_blur, thresh, lowest_scale, scale_up ? 1 : 0, d_scratch,
                               (SiftPointD *)d_pts, max_pts, num_pts_out);
  if (rc) return rc;
  return resolve_profile(ctx);
}

extern "C" int misift_extract_batch_u8(misift_ctx *ctx, const unsigned char *d_imgs, int nframes, size_t frame_stride,
                                       int width, int height, int pitch, int num_octaves, float init_blur,
                                       float thresh, float lowest_scale, float *d_scratch, void *d_pts, int max_pts,
                                       int *num_pts_out)
{
  ARG_CHECK(num_pts_out != nullptr);
  int rc = misift_extract_sync(ctx, d_imgs, 1, nframes, (long long)frame_stride, width, height, pitch, num_octaves,
                        init_blur, thresh, lowest_scale, 0, d_scratch, (SiftPointD *)d_pts, max_pts, num_pts_out);
  if (rc) return rc;
  return resolve_profile(ctx);
}

extern "C" int misift_extract_batch_async(misift_ctx *ctx, const float *d_imgs, int nframes, size_t frame_stride,
                                          int width, int height, int pitch, int num_octaves, float init_blur,
                                          float thresh, float lowest_scale, float *d_scratch, void *d_pts,
                                          int max_pts, int *d_counts_out)
{
  ARG_CHECK(ctx != nullptr);
  TinyScope tiny(ctx, width, height, num_octaves);
  int rc = misift_extract_enqueue(ctx, d_imgs, 0, nframes, (long long)frame_stride, width, height, pitch,
                                  num_octaves, init_blur, thresh, lowest_scale, 0, d_scratch, (SiftPointD *)d_pts,
                                  max_pts);
  if (rc) return rc;
  if (d_counts_out) return launch_export_counts(ctx, nframes, num_octaves, max_pts, d_counts_out, nullptr);
  return MISIFT_OK;
}

extern "C" int misift_extract_batch_packed_async(misift_ctx *ctx, const float *d_imgs, int nframes,
                                                 size_t frame_stride, int width, int height, int pitch,
                                                 int num_octaves, float init_blur, float thresh, float lowest_scale,
                                                 float *d_scratch, void *d_pts, int max_pts, int *d_counts_out,
                                                 int *d_offsets_out, void *d_packed_out)
{
  ARG_CHECK(ctx && d_counts_out && d_offsets_out && d_packed_out);
  TinyScope tiny(ctx, width, height, num_octaves);
  CtxExtra *px = extra(ctx);
  if (!px->lanes.empty()) {
    // batches in flight: this call goes to the next pipeline of the ring, behind a marker on the caller's stream
    const size_t k = px->lanes.size();
    misift_ctx *lane = px->lanes[px->ticket % k];
    hipEvent_t done = px->lane_done[px->ticket % (2 * k)];
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(px->ev_in, ctx->stream));
    HIP_TRY(hipStreamWaitEvent(lane->stream, px->ev_in, 0));
    lane->opt = ctx->opt;
    lane->profile = ctx->profile;
    const int rc = misift_extract_batch_packed_async(lane, d_imgs, nframes, frame_stride, width, height, pitch, num_octaves,
                                                     init_blur, thresh, lowest_scale, d_scratch, d_pts, max_pts, d_counts_out,
                                                     d_offsets_out, d_packed_out);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(done, lane->stream));
    px->last_lane = lane;
    px->last_done = done;
    px->ticket++;
    return MISIFT_OK;
  }
  if (ctx->opt.fused) {
    // merged-octave path: descr_all writes the packed array itself (no separate packing pass); d_pts may be NULL
    ctx->pack_counts = d_counts_out; ctx->pack_offsets = d_offsets_out; ctx->pack_dst = (SiftPointD *)d_packed_out;
    const int rc = misift_extract_enqueue(ctx, d_imgs, 0, nframes, (long long)frame_stride, width, height, pitch,
                                          num_octaves, init_blur, thresh, lowest_scale, 0, d_scratch,
                                          (SiftPointD *)d_pts, max_pts);
    ctx->pack_counts = nullptr; ctx->pack_offsets = nullptr; ctx->pack_dst = nullptr;
    return rc;
  }
  ARG_CHECK(d_pts != nullptr);
  int rc = misift_extract_enqueue(ctx, d_imgs, 0, nframes, (long long)frame_stride, width, height, pitch,
                                  num_octaves, init_blur, thresh, lowest_scale, 0, d_scratch, (SiftPointD *)d_pts,
                                  max_pts);
  if (rc) return rc;
  rc = launch_export_counts(ctx, nframes, num_octaves, max_pts, d_counts_out, d_offsets_out);
  if (rc) return rc;
  return launch_pack_records(ctx, (const SiftPointD *)d_pts, max_pts, nframes, d_offsets_out,
                             (SiftPointD *)d_packed_out);
}

extern "C" int misift_get_counters(misift_ctx *ctx, int frame, unsigned int *counters17)
{
  ARG_CHECK(ctx != nullptr);
  ctx = result_ctx(ctx);               // batches in flight: the pipeline that took the most recent batch
  ARG_CHECK(counters17 && frame >= 0 && frame < ctx->cap_frames);
  unsigned tmp[CNT_STRIDE];
  HIP_TRY(hipMemcpyAsync(tmp, ctx->d_counters + (size_t)frame * CNT_STRIDE, sizeof(tmp), hipMemcpyDeviceToHost,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  memcpy(counters17, tmp, sizeof(unsigned) * 17);
  return MISIFT_OK;
}

// Diagnostic: all CNT_STRIDE (64) words of one frame's counter block — the reference's 17 counters, then the library's
// own (candidates / detections / duplicates per octave, overflow flags); frame == number of frames of the last call
// reads the spare block that holds the call's flags.
extern "C" int misift_get_counter_block(misift_ctx *ctx, int frame, unsigned int *words64)
{
  ARG_CHECK(ctx != nullptr);
  ctx = result_ctx(ctx);
  ARG_CHECK(words64 && frame >= 0 && frame <= ctx->cap_frames);
  HIP_TRY(hipMemcpyAsync(words64, ctx->d_counters + (size_t)frame * CNT_STRIDE, sizeof(unsigned) * CNT_STRIDE,
                         hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_set_counters(misift_ctx *ctx, int frame, const unsigned int *counters17)
{
  ARG_CHECK(ctx && counters17 && frame >= 0 && frame < ctx->cap_frames);
  unsigned tmp[CNT_STRIDE];
  memset(tmp, 0, sizeof(tmp));
  memcpy(tmp, counters17, sizeof(unsigned) * 17);
  HIP_TRY(hipMemcpyAsync(ctx->d_counters + (size_t)frame * CNT_STRIDE, tmp, sizeof(tmp), hipMemcpyHostToDevice,
                         ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

// ------------------------------------------------------- stage entry points
extern "C" int misift_lowpass(misift_ctx *ctx, const float *d_src, int width, int height, int spitch, float *d_dst,
                              int dpitch, float sigma)
{
  ARG_CHECK(ctx && d_src && d_dst && width > 0 && height > 0 && spitch >= width && dpitch >= width);
  float k9[9];
  lowpass_taps(sigma, k9);
  StripGeom g = make_geom(ctx, width, height, spitch, 1, 0, width, height, 62);
  int rc = launch_lowpass(ctx, d_src, 0, g, d_dst, dpitch, 0, k9, nullptr);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_lowpass_scaledown(misift_ctx *ctx, const float *d_src, int width, int height, int spitch,
                                        float *d_dst, int dpitch, float sigma, float *d_dst2, int dpitch2)
{
  ARG_CHECK(ctx && d_src && d_dst && d_dst2 && width >= 4 && height >= 8 && spitch >= width && dpitch >= width &&
            dpitch2 >= width / 2);
  HIP_TRY(hipSetDevice(ctx->device));
  float k9[9], k5[5];
  lowpass_taps(sigma, k9);
  scaledown_taps(0.5f, k5);
  StripGeom g = make_geom(ctx, width, height, spitch, 1, 0, width, height, 60);
  int done = 0;
  int rc = launch_lowpass_down(ctx, d_src, 0, g, d_dst, dpitch, 0, k9, d_dst2, dpitch2, 0, k5, &done, nullptr);
  if (rc) return rc;
  if (!done) {
    misift_set_error("misift_lowpass_scaledown: shape not supported by the fused kernel (width %% 4, alignment)");
    return MISIFT_EINVAL;
  }
  return resolve_profile(ctx);
}

extern "C" int misift_scaledown(misift_ctx *ctx, const float *d_src, int width, int height, int spitch, float *d_dst,
                                int dpitch)
{
  ARG_CHECK(ctx && d_src && d_dst && width > 1 && height > 1 && spitch >= width && dpitch >= width / 2);
  float k5[5];
  scaledown_taps(0.5f, k5);
  StripGeom g = make_geom(ctx, width, height, spitch, 1, 0, width / 2, height / 2, 62);
  int rc = launch_scaledown(ctx, d_src, g, d_dst, dpitch, 0, k5);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_scaleup(misift_ctx *ctx, const float *d_src, int width, int height, int spitch, float *d_dst,
                              int dpitch)
{
  ARG_CHECK(ctx && d_src && d_dst && width > 0 && height > 0 && spitch >= width && dpitch >= 2 * width &&
            (dpitch & 1) == 0);
  int rc = launch_scaleup(ctx, d_src, 0, width, height, spitch, 0, 1, d_dst, dpitch, 0);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_laplace(misift_ctx *ctx, const float *d_base, int width, int height, int pitch, int num_octaves,
                              int octave, float *d_dog)
{
  ARG_CHECK(ctx && d_base && d_dog && width > 0 && height > 0 && pitch >= width);
  ARG_CHECK(num_octaves >= 1 && num_octaves <= MISIFT_MAX_OCTAVES && octave >= 1 && octave <= num_octaves);
  float table[8 * 12 * 16];
  misift_laplace_taps(num_octaves, table);
  StripGeom g = make_geom(ctx, width, height, pitch, 1, 0, width, height, 62);
  int rc = launch_laplace(ctx, d_base, g, d_dog, 0, octave_taps(table, octave));
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_reset_counters(misift_ctx *ctx, int max_pts)
{
  ARG_CHECK(ctx && max_pts >= 1);
  int rc = misift_ensure_frames(ctx, 1, 2 * (size_t)max_pts);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned) * CNT_STRIDE, ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_findpoints(misift_ctx *ctx, const float *d_dog, int width, int height, int pitch, float thresh,
                                 float edge_limit, float lowest_scale, float subsampling, int octave, void *d_pts,
                                 int max_pts)
{
  ARG_CHECK(ctx && d_dog && d_pts && width >= 16 && height >= 16 && pitch >= width && width < 16384 && height < 16384);
  ARG_CHECK(octave >= 1 && octave <= MISIFT_MAX_OCTAVES && max_pts >= 1);
  size_t cap = (size_t)width * height / 4;
  if (cap < 65536) cap = 65536;
  int rc = misift_ensure_frames(ctx, 1, cap);
  if (rc) return rc;
  StripGeom g = make_geom(ctx, width, height, pitch, 1, 0, width, height, 62);
  rc = launch_detect(ctx, d_dog, g, 0, thresh, octave);
  if (rc) return rc;
  if (ctx->opt.reference_cap) {
    rc = launch_refcap(ctx, width, height, 1, octave);
    if (rc) return rc;
  }
  rc = launch_refine(ctx, d_dog, 0, nullptr, 0, nullptr, width, height, pitch, 1, thresh, edge_limit, 1.0f / NUM_SCALES,
                     lowest_scale, subsampling, octave, (SiftPointD *)d_pts, max_pts);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_dog_findpoints(misift_ctx *ctx, const float *d_base, int width, int height, int pitch,
                                     int num_octaves, int octave, float thresh, float edge_limit, float lowest_scale,
                                     float subsampling, void *d_pts, int max_pts)
{
  ARG_CHECK(ctx && d_base && d_pts && width >= 16 && height >= 16 && pitch >= width && width < 16384 && height < 16384);
  ARG_CHECK(num_octaves >= 1 && num_octaves <= MISIFT_MAX_OCTAVES && octave >= 1 && octave <= num_octaves);
  size_t cap = (size_t)width * height / 4;
  if (cap < 65536) cap = 65536;
  int rc = misift_ensure_frames(ctx, 1, cap);
  if (rc) return rc;
  float table[8 * 12 * 16];
  misift_laplace_taps(num_octaves, table);
  const LaplaceTaps taps = octave_taps(table, octave);
  StripGeom g = make_geom(ctx, width, height, pitch, 1, 0, width, height, 60);
  rc = launch_dog_scan(ctx, d_base, g, taps, thresh, octave);
  if (rc) return rc;
  rc = launch_refine(ctx, nullptr, 0, d_base, 0, &taps, width, height, pitch, 1, thresh, edge_limit, 1.0f / NUM_SCALES,
                     lowest_scale, subsampling, octave, (SiftPointD *)d_pts, max_pts);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_orientations(misift_ctx *ctx, const float *d_base, int width, int height, int pitch, int octave,
                                   void *d_pts, int max_pts)
{
  ARG_CHECK(ctx && d_base && d_pts && width > 0 && height > 0 && pitch >= width && octave >= 1 &&
            octave <= MISIFT_MAX_OCTAVES);
  int rc = launch_orient(ctx, d_base, 0, width, height, pitch, 1, octave, (SiftPointD *)d_pts, max_pts);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_descriptors(misift_ctx *ctx, const float *d_base, int width, int height, int pitch,
                                  float subsampling, int octave, void *d_pts, int max_pts)
{
  ARG_CHECK(ctx && d_base && d_pts && width > 0 && height > 0 && pitch >= width && octave >= 1 &&
            octave <= MISIFT_MAX_OCTAVES);
  int rc = launch_descr(ctx, d_base, 0, width, height, pitch, 1, subsampling, octave, (SiftPointD *)d_pts, max_pts);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

// Test-only: evaluate the DEVICE copy of one written-out elementary function on n inputs (0 = det_exp2(x),
// 1 = det_atan2(y, x), 2 = det_exp(x), 3 = det_sincos(x) -> out = sin, out2 = cos).  The kernels and the oracle share
// these expressions, so parity tests cannot see an error in them; tests/test_gpu_parity.py checks the bits against the
// oracle's copy and tests/test_oracle_cpu.py the values against float64 libm.
extern "C" int misift_test_elementary(misift_ctx *ctx, int fn, const float *d_x, const float *d_y, float *d_out,
                                      float *d_out2, int n)
{
  ARG_CHECK(ctx && fn >= 0 && fn <= 3 && d_x && d_out && n >= 0 && (fn != 1 || d_y) && (fn != 3 || d_out2));
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0) return MISIFT_OK;
  int rc = fn == 0 ? launch_test_exp2(ctx, d_x, d_out, n) : launch_test_points_fn(ctx, fn, d_x, d_y, d_out, d_out2, n);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_rescale_positions(misift_ctx *ctx, void *d_pts, int npts, float scale)
{
  ARG_CHECK(ctx && d_pts && npts >= 0);
  int rc = launch_rescale(ctx, (SiftPointD *)d_pts, npts, scale);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return MISIFT_OK;
}

// ----------------------------------------------------------------- matching
extern "C" int misift_match_rows(misift_ctx *ctx, void *d_pts1, int row_begin, int row_count, const void *d_pts2, int n2)
{
  ARG_CHECK(ctx && row_begin >= 0 && row_count >= 0 && n2 >= 0);
  if (row_count == 0 || n2 == 0) return MISIFT_OK;       // matching.cu:1095-1096
  ARG_CHECK(d_pts1 && d_pts2);
  RoctxRange range("misift_match");
  HIP_TRY(hipSetDevice(ctx->device));
  ctx->want_match_flag = 1;
  ctx->match_flagged = 0;
  int rc = launch_match(ctx, (SiftPointD *)d_pts1, row_begin, row_count, (const SiftPointD *)d_pts2, n2);
  ctx->want_match_flag = 0;
  if (rc) return rc;
  if (ctx->match_flagged) rc = wait_host_flag(ctx, ctx->h_flags, ctx->match_seq);      // matching.cu:1191
  else HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (rc) return rc;
  return resolve_profile(ctx);
}

// Test-only: the two-launch column split of the sharded matcher (multigpu.hip) on one set-2 buffer — super-tiles
// [own_tile_begin, own_tile_end) first, the rest second, one merge — so its result bits and its cost can be checked
// without a communicator.
extern "C" int misift_test_match_split(misift_ctx *ctx, void *d_pts1, int n1, const void *d_pts2, int n2,
                                       int own_tile_begin, int own_tile_end)
{
  ARG_CHECK(ctx && n1 >= 0 && n2 >= 0 && own_tile_begin >= 0 && own_tile_end >= own_tile_begin);
  if (n1 == 0 || n2 == 0) return MISIFT_OK;
  ARG_CHECK(d_pts1 && d_pts2);
  HIP_TRY(hipSetDevice(ctx->device));
  int rc = launch_match_split(ctx, (SiftPointD *)d_pts1, 0, n1, (const SiftPointD *)d_pts2, n2,
                              (const SiftPointD *)d_pts2, own_tile_begin, own_tile_end, nullptr, MATCH_PHASE_ALL, 0);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return resolve_profile(ctx);
}

extern "C" int misift_match(misift_ctx *ctx, void *d_pts1, int n1, const void *d_pts2, int n2)
{
  return misift_match_rows(ctx, d_pts1, 0, n1, d_pts2, n2);
}

// The next slot of the pinned ring for a batch call's host lists, holding at least `bytes`: it waits for the call that
// last used the slot (mb_done), so the caller may copy its lists in and must record mb_done[*slot] behind its launches.
static int mb_ring_slot(misift_ctx *ctx, size_t bytes, int *slot_out)
{
  CtxExtra *x = extra(ctx);
  const int slot = (int)(x->mb_next++ % CtxExtra::MB_RING);
  if (x->mb_done[slot]) HIP_TRY(hipEventSynchronize(x->mb_done[slot]));
  else HIP_TRY(hipEventCreateWithFlags(&x->mb_done[slot], hipEventDisableTiming));
  if (bytes > x->mb_pairs_cap[slot]) {
    if (x->mb_pairs[slot]) HIP_TRY(hipHostFree(x->mb_pairs[slot]));
    x->mb_pairs[slot] = nullptr; x->mb_pairs_cap[slot] = 0;
    HIP_TRY(hipHostMalloc((void **)&x->mb_pairs[slot], bytes, hipHostMallocDefault));
    x->mb_pairs_cap[slot] = bytes;
  }
  *slot_out = slot;
  return MISIFT_OK;
}

// Test-only, host state only (no HIP call, no sync): what a test of the shared temp and the ring reasons about.
extern "C" long long misift_test_ctx_state(misift_ctx *ctx, int which)
{
  if (!ctx || which < 0 || which > 2) {
    misift_set_error("misift_test_ctx_state: invalid argument");
    return MISIFT_EINVAL;
  }
  if (which == 0) return (long long)ctx->match_tmp_bytes;
  if (which == 1) return CtxExtra::MB_RING;
  return (long long)extra(ctx)->mb_next;
}

// The device plan of misift_match_batch / misift_match_batch_i8 (grow-only, stream-ordered like the calls that use it).
static int ensure_mb_plan(misift_ctx *ctx, size_t bytes)
{
  CtxExtra *x = extra(ctx);
  if (bytes > x->mb_plan_bytes) {
    if (x->d_mb_plan) {
      HIP_TRY(hipStreamSynchronize(ctx->stream));
      HIP_TRY(misift_dev_free(x->d_mb_plan));
    }
    x->d_mb_plan = nullptr; x->mb_plan_bytes = 0;
    HIP_TRY(misift_dev_alloc(&x->d_mb_plan, bytes, "match_batch_plan"));
    x->mb_plan_bytes = bytes;
  }
  return MISIFT_OK;
}

// The checks of the batch calls, made before anything is enqueued; an error names the entry point `who`.
// One set of records: without offsets, frame f starts at record f * stride.
static int batch_layout(const char *who, const void *recs, const int *counts, const int *offsets, int stride,
                        BatchLayout *set)
{
  ARG_CHECK_IN(who, offsets || stride >= 0);
  *set = BatchLayout{(SiftPointD *)recs, counts, offsets, stride};
  return MISIFT_OK;
}

// A list of n entries of `step` ints: a frame of the first batch (nframes1 frames), and for pairs (step 2) a frame of
// the second (nframes2 frames).  Every index in range; a frame of the first batch in at most one entry unless `repeats`.
static int check_frames(const char *who, int n, const int *list, int step, int nframes1, int nframes2,
                        bool repeats = false)
{
  std::vector<char> taken((size_t)nframes1, 0);
  for (int i = 0; i < n; i++) {
    const int f1 = list[step * i], f2 = step == 2 ? list[step * i + 1] : 0;
    ARG_CHECK_IN(who, f1 >= 0 && f1 < nframes1 && (step == 1 || (f2 >= 0 && f2 < nframes2)));
    if (repeats) continue;
    ARG_CHECK_IN(who, !taken[f1]);
    taken[f1] = 1;
  }
  return MISIFT_OK;
}

// The host side of a batch call, behind its checks: the caller's host lists go, in order, to the next slot of the pinned
// ring; plan_bytes > 0 provides the device plan of the pair matchers; launch(slot, plan) enqueues the launches, and
// mb_done of the slot is recorded behind them, also when a launch failed.
struct HostList {
  const void *src;
  size_t bytes;
};
template <class Launch>
static int run_batch(misift_ctx *ctx, std::initializer_list<HostList> lists, size_t plan_bytes, Launch launch)
{
  HIP_TRY(hipSetDevice(ctx->device));
  CtxExtra *x = extra(ctx);
  size_t bytes = 0;
  for (const HostList &l : lists) bytes += l.bytes;
  int slot;
  int rc = mb_ring_slot(ctx, bytes, &slot);
  if (rc) return rc;
  char *h = reinterpret_cast<char *>(x->mb_pairs[slot]);
  for (const HostList &l : lists) {
    if (l.bytes) memcpy(h, l.src, l.bytes);
    h += l.bytes;
  }
  if (plan_bytes) {
    rc = ensure_mb_plan(ctx, plan_bytes);
    if (rc) return rc;
  }
  rc = launch(x->mb_pairs[slot], x->d_mb_plan);
  HIP_TRY(hipEventRecord(x->mb_done[slot], ctx->stream));
  return rc;
}

// The four pair matchers share everything but the checks that are an entry point's own.  One side of a call:
struct PairSide {
  const void *recs;
  int nframes;
  const int *counts, *offsets;
  int stride;
};
// own_failed: NULL, or the text of the entry point's own check that failed; it is reported in its place, behind the
// common NULL and range checks.  Then the layouts, the frames of the pairs (a frame of set 1 in at most one pair unless
// `repeats`), and launch(h_pairs, d_plan, set1, set2) through run_batch with the pairs' device plan.
#define OWN_CHECK(cond) ((cond) ? nullptr : #cond)
static int own_check_failed(const char *who, const char *text)
{
  misift_set_error("%s: invalid argument: %s", who, text);
  return MISIFT_EINVAL;
}
template <class Launch>
static int pair_match_call(const char *who, misift_ctx *ctx, int npairs, const int *pairs, const PairSide &s1,
                           const PairSide &s2, const char *own_failed, bool repeats, Launch launch)
{
  ARG_CHECK_IN(who, ctx && npairs >= 0);
  if (npairs == 0) return MISIFT_OK;
  ARG_CHECK_IN(who, pairs && s1.recs && s2.recs && s1.counts && s2.counts && s1.nframes > 0 && s2.nframes > 0);
  if (own_failed) return own_check_failed(who, own_failed);
  BatchLayout set1, set2;
  int rc = batch_layout(who, s1.recs, s1.counts, s1.offsets, s1.stride, &set1);
  if (!rc) rc = batch_layout(who, s2.recs, s2.counts, s2.offsets, s2.stride, &set2);
  if (!rc) rc = check_frames(who, npairs, pairs, 2, s1.nframes, s2.nframes, repeats);
  if (rc) return rc;
  RoctxRange range(who);
  return run_batch(ctx, {{pairs, sizeof(int) * 2 * (size_t)npairs}}, pair_plan_bytes(npairs),
                   [&](int *h_pairs, void *d_plan) { return launch(h_pairs, d_plan, set1, set2); });
}

// Many (frame of set 1, frame of set 2) pairs of device-resident batches in one stream-ordered call: no host wait and no
// host read of the counts.
extern "C" int misift_match_batch(misift_ctx *ctx, int npairs, const int *pairs, void *d_recs1, int nframes1,
                                  const int *d_counts1, const int *d_offsets1, int stride1, const void *d_recs2,
                                  int nframes2, const int *d_counts2, const int *d_offsets2, int stride2)
{
  const PairSide s1{d_recs1, nframes1, d_counts1, d_offsets1, stride1};
  const PairSide s2{d_recs2, nframes2, d_counts2, d_offsets2, stride2};
  return pair_match_call(__func__, ctx, npairs, pairs, s1, s2, nullptr, false,
                        [&](int *h_pairs, void *d_plan, const BatchLayout &set1, const BatchLayout &set2) {
                          return launch_match_batch(ctx, PAIR_OUT_INPLACE, npairs, h_pairs, d_plan, set1, set2,
                                                    PairRows{});
                        });
}

// misift_match_batch into pair-indexed output rows, with an optional mutual-nearest-neighbour check: frames may repeat.
extern "C" int misift_match_pairs_batch(misift_ctx *ctx, int npairs, const int *pairs, const void *d_recs1,
                                        int nframes1, const int *d_counts1, const int *d_offsets1, int stride1,
                                        const void *d_recs2, int nframes2, const int *d_counts2, const int *d_offsets2,
                                        int stride2, int max_pts, int mutual, void *d_out, int *d_out_counts,
                                        int *d_num_matched)
{
  const PairSide s1{d_recs1, nframes1, d_counts1, d_offsets1, stride1};
  const PairSide s2{d_recs2, nframes2, d_counts2, d_offsets2, stride2};
  const PairRows rows{max_pts, d_out, d_out_counts, d_num_matched};
  const char *own = OWN_CHECK(d_out && d_out_counts && max_pts >= 1 && (mutual == 0 || mutual == 1) &&
                              d_out != d_recs1 && d_out != d_recs2);
  return pair_match_call(__func__, ctx, npairs, pairs, s1, s2, own, true,
                        [&](int *h_pairs, void *d_plan, const BatchLayout &set1, const BatchLayout &set2) {
                          return launch_match_batch(ctx, mutual ? PAIR_OUT_MUTUAL : PAIR_OUT_INDEXED, npairs, h_pairs,
                                                    d_plan, set1, set2, rows);
                        });
}

// The seven frame-list calls (one entry per selected frame of one set of records) share everything but the checks that are
// an entry point's own; the counterpart of pair_match_call.  null_failed: NULL, or the text of the entry point's own NULL
// check that failed.  own(): evaluated behind the NULL checks and the layout only, NULL or the text of the entry point's
// own check that failed.  Then the frames of the list (each frame in at most one entry), and launch(h_frames, h_extra,
// set) through run_batch, h_extra being the pinned copy of the entry point's second host list `extra` (may be empty).
template <class Own, class Launch>
static int frame_list_call(const char *who, misift_ctx *ctx, int nsel, const int *frames, const PairSide &s,
                           const char *null_failed, HostList extra, Own own, Launch launch)
{
  ARG_CHECK_IN(who, ctx && nsel >= 0);
  if (nsel == 0) return MISIFT_OK;
  ARG_CHECK_IN(who, frames && s.recs && s.counts && s.nframes > 0);
  if (null_failed) return own_check_failed(who, null_failed);
  BatchLayout set;
  int rc = batch_layout(who, s.recs, s.counts, s.offsets, s.stride, &set);
  if (rc) return rc;
  if (const char *failed = own()) return own_check_failed(who, failed);
  rc = check_frames(who, nsel, frames, 1, s.nframes, 0);
  if (rc) return rc;
  RoctxRange range(who);
  return run_batch(ctx, {{frames, sizeof(int) * (size_t)nsel}, extra}, 0,
                   [&](int *h_frames, void *) { return launch(h_frames, (const void *)(h_frames + nsel), set); });
}

// Many frames of a device-resident batch through FindHomography / ImproveHomography in one stream-ordered call each: no
// host wait and no host read of the counts.
extern "C" int misift_find_homography_batch(misift_ctx *ctx, int nsel, const int *frames, const unsigned *seeds,
                                            const void *d_recs, int nframes, const int *d_counts, const int *d_offsets,
                                            int stride, int max_pts, int num_loops, float min_score,
                                            float max_ambiguity, float thresh, float *d_homography, int *d_num_matches)
{
  const PairSide s{d_recs, nframes, d_counts, d_offsets, stride};
  return frame_list_call(
      __func__, ctx, nsel, frames, s, OWN_CHECK(seeds && d_homography && d_num_matches),
      HostList{seeds, sizeof(unsigned) * (size_t)nsel}, [&] { return OWN_CHECK(num_loops >= 1 && max_pts >= 1); },
      [&](const int *h_frames, const void *h_seeds, const BatchLayout &set) {
        return launch_find_homography_batch(ctx, nsel, h_frames, (const unsigned *)h_seeds, set, max_pts, num_loops,
                                            min_score, max_ambiguity, thresh, d_homography, d_num_matches);
      });
}

extern "C" int misift_improve_homography_batch(misift_ctx *ctx, int nsel, const int *frames, void *d_recs, int nframes,
                                               const int *d_counts, const int *d_offsets, int stride, int num_loops,
                                               float min_score, float max_ambiguity, float thresh, float *d_homography,
                                               int *d_num_fit)
{
  const PairSide s{d_recs, nframes, d_counts, d_offsets, stride};
  return frame_list_call(
      __func__, ctx, nsel, frames, s, OWN_CHECK(d_homography && d_num_fit), HostList{},
      [&] { return OWN_CHECK(num_loops >= 0); },
      [&](const int *h_frames, const void *, const BatchLayout &set) {
        return launch_improve_homography_batch(ctx, nsel, h_frames, set, num_loops, min_score, max_ambiguity, thresh,
                                               d_homography, d_num_fit);
      });
}

// The epipolar counterpart: a RANSAC fundamental matrix per frame, and the Sampson distance of every record under a
// given F into match_error, in one stream-ordered call each.
extern "C" int misift_find_fundamental_batch(misift_ctx *ctx, int nsel, const int *frames, const unsigned *seeds,
                                             const void *d_recs, int nframes, const int *d_counts, const int *d_offsets,
                                             int stride, int max_pts, int num_loops, float min_score,
                                             float max_ambiguity, float thresh, float *d_fundamental,
                                             int *d_num_inliers)
{
  const PairSide s{d_recs, nframes, d_counts, d_offsets, stride};
  return frame_list_call(
      __func__, ctx, nsel, frames, s, OWN_CHECK(seeds && d_fundamental && d_num_inliers),
      HostList{seeds, sizeof(unsigned) * (size_t)nsel},
      [&] { return OWN_CHECK(num_loops >= 1 && max_pts >= 1 && thresh > 0.0f); },
      [&](const int *h_frames, const void *h_seeds, const BatchLayout &set) {
        return launch_find_fundamental_batch(ctx, nsel, h_frames, (const unsigned *)h_seeds, set, max_pts, num_loops,
                                             min_score, max_ambiguity, thresh, d_fundamental, d_num_inliers);
      });
}

extern "C" int misift_score_fundamental_batch(misift_ctx *ctx, int nsel, const int *frames, void *d_recs, int nframes,
                                              const int *d_counts, const int *d_offsets, int stride, float min_score,
                                              float max_ambiguity, float thresh, const float *d_fundamental,
                                              int *d_num_fit)
{
  const PairSide s{d_recs, nframes, d_counts, d_offsets, stride};
  return frame_list_call(
      __func__, ctx, nsel, frames, s, OWN_CHECK(d_fundamental && d_num_fit), HostList{},
      [&] { return OWN_CHECK(thresh > 0.0f); },
      [&](const int *h_frames, const void *, const BatchLayout &set) {
        return launch_score_fundamental_batch(ctx, nsel, h_frames, set, min_score, max_ambiguity, thresh,
                                              d_fundamental, d_num_fit);
      });
}

// Refits of each frame's F over its inliers, then match_error under the result: the epipolar counterpart of
// misift_improve_homography_batch.
extern "C" int misift_improve_fundamental_batch(misift_ctx *ctx, int nsel, const int *frames, void *d_recs, int nframes,
                                                const int *d_counts, const int *d_offsets, int stride, int num_loops,
                                                float min_score, float max_ambiguity, float thresh,
                                                float *d_fundamental, int *d_num_fit, int *d_num_rounds)
{
  const PairSide s{d_recs, nframes, d_counts, d_offsets, stride};
  return frame_list_call(
      __func__, ctx, nsel, frames, s, OWN_CHECK(d_fundamental && d_num_fit), HostList{},
      [&] { return OWN_CHECK(num_loops >= 0 && thresh > 0.0f); },
      [&](const int *h_frames, const void *, const BatchLayout &set) {
        return launch_improve_fundamental_batch(ctx, nsel, h_frames, set, num_loops, min_score, max_ambiguity, thresh,
                                                d_fundamental, d_num_fit, d_num_rounds);
      });
}

// fx fy cx cy of `cameras` cameras: focal lengths finite and > 0, principal points finite
static bool intrinsics_usable(const float *k, int cameras = 2)
{
  for (int c = 0; c < 4 * cameras; c += 4) {
    if (!(k[c] > 0.0f && k[c + 1] > 0.0f && std::isfinite(k[c]) && std::isfinite(k[c + 1]))) return false;
    if (!(std::isfinite(k[c + 2]) && std::isfinite(k[c + 3]))) return false;
  }
  return true;
}

// The relative pose of each frame pair from its F and its intrinsics, and the two-view depth of every record: the pose
// counterpart of misift_score_fundamental_batch.
extern "C" int misift_recover_pose_batch(misift_ctx *ctx, int nsel, const int *frames, const float *intrinsics,
                                         const void *d_recs, int nframes, const int *d_counts, const int *d_offsets,
                                         int stride, float min_score, float max_ambiguity, float thresh,
                                         const float *d_fundamental, float *d_pose, int *d_num_front, int *d_votes,
                                         float *d_xyz)
{
  const PairSide s{d_recs, nframes, d_counts, d_offsets, stride};
  return frame_list_call(
      __func__, ctx, nsel, frames, s, OWN_CHECK(intrinsics && d_fundamental && d_pose && d_num_front),
      HostList{intrinsics, sizeof(float) * 8 * (size_t)nsel},
      [&]() -> const char * {
        for (int i = 0; i < nsel; i++)
          if (!intrinsics_usable(intrinsics + (size_t)8 * i)) return "intrinsics_usable(intrinsics + (size_t)8 * i)";
        return OWN_CHECK(thresh > 0.0f);
      },
      [&](const int *h_frames, const void *h_intrinsics, const BatchLayout &set) {
        return launch_recover_pose_batch(ctx, nsel, h_frames, (const float *)h_intrinsics, set, min_score,
                                         max_ambiguity, thresh, d_fundamental, d_pose, d_num_front, d_votes, d_xyz);
      });
}

// Behind misift_recover_pose_batch: the pose of each frame pair that is planar or rotation-only from its homography,
// written over that call's outputs; every other entry is left alone.
extern "C" int misift_recover_pose_planar_batch(misift_ctx *ctx, int nsel, const int *frames, const float *intrinsics,
                                                const void *d_recs, int nframes, const int *d_counts,
                                                const int *d_offsets, int stride, float min_score, float max_ambiguity,
                                                float thresh_h, float thresh_f, float planar_ratio, int min_inliers,
                                                float min_baseline, const float *d_homography,
                                                const float *d_fundamental, int *d_model, int *d_hf_counts,
                                                float *d_pose, int *d_num_front, int *d_votes, float *d_xyz,
                                                float *d_pose_alt, float *d_plane)
{
  const PairSide s{d_recs, nframes, d_counts, d_offsets, stride};
  return frame_list_call(
      __func__, ctx, nsel, frames, s,
      OWN_CHECK(intrinsics && d_homography && d_model && d_hf_counts && d_pose && d_num_front),
      HostList{intrinsics, sizeof(float) * 8 * (size_t)nsel},
      [&]() -> const char * {
        for (int i = 0; i < nsel; i++)
          if (!intrinsics_usable(intrinsics + (size_t)8 * i)) return "intrinsics_usable(intrinsics + (size_t)8 * i)";
        return OWN_CHECK(thresh_h > 0.0f && thresh_f > 0.0f && planar_ratio >= 0.0f && min_inliers >= 4 &&
                         min_baseline >= 0.0f);                   // a NaN fails each
      },
      [&](const int *h_frames, const void *h_intrinsics, const BatchLayout &set) {
        const PlanarPoseParams p{min_score, max_ambiguity, thresh_h, thresh_f, planar_ratio, min_inliers, min_baseline};
        const PlanarPoseOut out{d_model, d_hf_counts, d_pose, d_num_front, d_votes, d_xyz, d_pose_alt, d_plane};
        return launch_recover_pose_planar_batch(ctx, nsel, h_frames, (const float *)h_intrinsics, set, p, d_homography,
                                                d_fundamental, out);
      });
}

// Homography- and epipolar-guided matching of many frame pairs in one stream-ordered call each: no host wait and no host
// read of the counts.  The host lists: the pairs, each pair's index among the distinct set-2 frames, and those frames.
// d_model: the pairs' homographies (epipolar false) or fundamental matrices (true).
static int match_gated_batch(const char *fn, bool epipolar, misift_ctx *ctx, int npairs, const int *pairs, void *d_recs1,
                             int nframes1, const int *d_counts1, const int *d_offsets1, int stride1,
                             const void *d_recs2, int nframes2, const int *d_counts2, const int *d_offsets2,
                             int stride2, const float *d_model, float radius, int max_pts, int *d_num_found)
{
  ARG_CHECK_IN(fn, ctx && npairs >= 0);
  if (npairs == 0) return MISIFT_OK;
  ARG_CHECK_IN(fn, pairs && d_recs1 && d_recs2 && d_counts1 && d_counts2 && d_model && nframes1 > 0 && nframes2 > 0);
  BatchLayout set1, set2;
  int rc = batch_layout(fn, d_recs1, d_counts1, d_offsets1, stride1, &set1);
  if (!rc) rc = batch_layout(fn, d_recs2, d_counts2, d_offsets2, stride2, &set2);
  if (rc) return rc;
  ARG_CHECK_IN(fn, radius > 0.0f);                                // NaN fails too
  ARG_CHECK_IN(fn, max_pts >= 1);
  rc = check_frames(fn, npairs, pairs, 2, nframes1, nframes2);
  if (rc) return rc;
  std::vector<int> dindex((size_t)nframes2, -1), pair_d((size_t)npairs), distinct;
  for (int p = 0; p < npairs; p++) {
    const int f2 = pairs[2 * p + 1];
    if (dindex[f2] < 0) {
      dindex[f2] = (int)distinct.size();
      distinct.push_back(f2);
    }
    pair_d[p] = dindex[f2];
  }
  const int nd = (int)distinct.size();
  RoctxRange range(fn);
  return run_batch(ctx,
                   {{pairs, sizeof(int) * 2 * (size_t)npairs},
                    {pair_d.data(), sizeof(int) * (size_t)npairs},
                    {distinct.data(), sizeof(int) * (size_t)nd}},
                   0, [&](int *h_pairs, void *) {
                     const int *h_pair_d = h_pairs + 2 * (size_t)npairs;
                     return (epipolar ? launch_match_epipolar_batch : launch_match_guided_batch)(
                         ctx, npairs, h_pairs, h_pair_d, h_pair_d + npairs, nd, set1, set2, d_model, radius, max_pts,
                         d_num_found);
                   });
}

extern "C" int misift_match_guided_batch(misift_ctx *ctx, int npairs, const int *pairs, void *d_recs1, int nframes1,
                                         const int *d_counts1, const int *d_offsets1, int stride1, const void *d_recs2,
                                         int nframes2, const int *d_counts2, const int *d_offsets2, int stride2,
                                         const float *d_homography, float radius, int max_pts, int *d_num_found)
{
  return match_gated_batch(__func__, false, ctx, npairs, pairs, d_recs1, nframes1, d_counts1, d_offsets1, stride1,
                           d_recs2, nframes2, d_counts2, d_offsets2, stride2, d_homography, radius, max_pts, d_num_found);
}

extern "C" int misift_match_epipolar_batch(misift_ctx *ctx, int npairs, const int *pairs, void *d_recs1, int nframes1,
                                           const int *d_counts1, const int *d_offsets1, int stride1, const void *d_recs2,
                                           int nframes2, const int *d_counts2, const int *d_offsets2, int stride2,
                                           const float *d_fundamental, float radius, int max_pts, int *d_num_found)
{
  return match_gated_batch(__func__, true, ctx, npairs, pairs, d_recs1, nframes1, d_counts1, d_offsets1, stride1,
                           d_recs2, nframes2, d_counts2, d_offsets2, stride2, d_fundamental, radius, max_pts,
                           d_num_found);
}

// 8-bit descriptors of every record of a device-resident batch, one stream-ordered launch with the counts on the device.
extern "C" int misift_quantize_batch(misift_ctx *ctx, const void *d_recs, int nframes, const int *d_counts,
                                     const int *d_offsets, int stride, int8_t *d_q)
{
  ARG_CHECK(ctx && d_recs && d_counts && d_q && nframes >= 0);
  ARG_CHECK(((uintptr_t)d_q & 15) == 0);
  BatchLayout set;
  int rc = batch_layout(__func__, d_recs, d_counts, d_offsets, stride, &set);
  if (rc) return rc;
  if (nframes == 0) return MISIFT_OK;
  RoctxRange range(__func__);
  HIP_TRY(hipSetDevice(ctx->device));
  return launch_quantize_batch(ctx, set, nframes, d_q);
}

// misift_match_batch on 8-bit descriptors (int8 matrix cores): the same pairs, layouts, checks and stream semantics.
extern "C" int misift_match_batch_i8(misift_ctx *ctx, int npairs, const int *pairs, void *d_recs1, const int8_t *d_q1,
                                     int nframes1, const int *d_counts1, const int *d_offsets1, int stride1,
                                     const void *d_recs2, const int8_t *d_q2, int nframes2, const int *d_counts2,
                                     const int *d_offsets2, int stride2)
{
  const PairSide s1{d_recs1, nframes1, d_counts1, d_offsets1, stride1};
  const PairSide s2{d_recs2, nframes2, d_counts2, d_offsets2, stride2};
  const char *own = OWN_CHECK(d_q1 && d_q2 && ((uintptr_t)d_q1 & 15) == 0 && ((uintptr_t)d_q2 & 15) == 0);
  return pair_match_call(__func__, ctx, npairs, pairs, s1, s2, own, false,
                        [&](int *h_pairs, void *d_plan, const BatchLayout &set1, const BatchLayout &set2) {
                          return launch_match_batch_i8(ctx, PAIR_OUT_INPLACE, npairs, h_pairs, d_plan, set1, d_q1, set2,
                                                       d_q2, PairRows{});
                        });
}

// misift_match_pairs_batch with the scores of misift_match_batch_i8: pair-indexed output rows, optional mutual check.
extern "C" int misift_match_pairs_batch_i8(misift_ctx *ctx, int npairs, const int *pairs, const void *d_recs1,
                                           const int8_t *d_q1, int nframes1, const int *d_counts1,
                                           const int *d_offsets1, int stride1, const void *d_recs2, const int8_t *d_q2,
                                           int nframes2, const int *d_counts2, const int *d_offsets2, int stride2,
                                           int max_pts, int mutual, void *d_out, int *d_out_counts, int *d_num_matched)
{
  const PairSide s1{d_recs1, nframes1, d_counts1, d_offsets1, stride1};
  const PairSide s2{d_recs2, nframes2, d_counts2, d_offsets2, stride2};
  const PairRows rows{max_pts, d_out, d_out_counts, d_num_matched};
  const char *own = OWN_CHECK(d_q1 && d_q2 && ((uintptr_t)d_q1 & 15) == 0 && ((uintptr_t)d_q2 & 15) == 0);
  if (!own)
    own = OWN_CHECK(d_out && d_out_counts && max_pts >= 1 && (mutual == 0 || mutual == 1) && d_out != d_recs1 &&
                    d_out != d_recs2);
  return pair_match_call(__func__, ctx, npairs, pairs, s1, s2, own, true,
                        [&](int *h_pairs, void *d_plan, const BatchLayout &set1, const BatchLayout &set2) {
                          return launch_match_batch_i8(ctx, mutual ? PAIR_OUT_MUTUAL : PAIR_OUT_INDEXED, npairs,
                                                       h_pairs, d_plan, set1, d_q1, set2, d_q2, rows);
                        });
}

// The accepted matches of a pair-indexed batch joined across pairs into feature tracks: connected components over the
// global record indices of one batch, labelled by their smallest member.  Only the rows, the counts and the offsets are
// read.
extern "C" int misift_link_tracks_batch(misift_ctx *ctx, int npairs, const int *pairs, const void *d_rows,
                                        const int *d_row_counts, int max_pts, int nframes, const int *d_counts,
                                        const int *d_offsets, int stride, int max_records, float min_score,
                                        float max_ambiguity, float max_error, int *d_track, int *d_track_len,
                                        int *d_track_frames, int *d_summary)
{
  ARG_CHECK(ctx && npairs >= 0 && nframes >= 0);
  ARG_CHECK((pairs || npairs == 0) && d_rows && d_row_counts && d_counts);
  ARG_CHECK(d_track && d_track_len && d_track_frames && d_summary);
  ARG_CHECK(max_pts >= 1 && max_records >= 1);
  ARG_CHECK(min_score == min_score && max_ambiguity == max_ambiguity);      // not NaN
  ARG_CHECK(max_error > 0.0f);                                              // NaN fails too
  BatchLayout set;
  int rc = batch_layout(__func__, nullptr, d_counts, d_offsets, stride, &set);
  if (!rc) rc = check_frames(__func__, npairs, pairs, 2, nframes, nframes, true);
  if (rc) return rc;
  RoctxRange range(__func__);
  static const int no_pair[2] = {0, 0};                                     // npairs == 0: the list slot is never read
  const HostList list = npairs ? HostList{pairs, sizeof(int) * 2 * (size_t)npairs} : HostList{no_pair, sizeof(no_pair)};
  return run_batch(ctx, {list}, 0, [&](int *h_pairs, void *) {
    return launch_link_tracks_batch(ctx, npairs, h_pairs, d_rows, d_row_counts, max_pts, set, nframes, max_records,
                                    min_score, max_ambiguity, max_error, d_track, d_track_len, d_track_frames,
                                    d_summary);
  });
}

// Preemptive matching: the frame pairs worth matching, chosen on the device from the `top` largest-scale features of
// every frame (kernels_select.hip; the rules are select_core.hpp).  The byte ranges the host knows: every output, the
// counts, the offsets and, in a padded layout, the records and their q; of a packed layout's records and q only the
// first byte, since their extent is device data.
extern "C" int misift_select_pairs_batch(misift_ctx *ctx, const void *d_recs, const int8_t *d_q, int nframes,
                                         const int *d_counts, const int *d_offsets, int stride, int top, float min_score,
                                         float max_ambiguity, int min_votes, int k, int max_pairs, int *d_sel,
                                         int *d_sel_counts, int *d_votes, int *d_pairs, int *d_pair_votes, int *d_summary)
{
  ARG_CHECK(ctx && d_recs && d_q && d_counts);
  ARG_CHECK(d_sel && d_sel_counts && d_votes && d_pairs && d_pair_votes && d_summary);
  ARG_CHECK(((uintptr_t)d_q & 15) == 0);
  ARG_CHECK(nframes >= 0 && nframes <= MISIFT_SELECT_MAX_FRAMES);
  ARG_CHECK(top >= 1 && top <= MISIFT_SELECT_MAX_TOP && k >= 1 && min_votes >= 1 && max_pairs >= 0);
  ARG_CHECK(min_score == min_score && max_ambiguity == max_ambiguity);      // not NaN
  BatchLayout set;
  int rc = batch_layout(__func__, d_recs, d_counts, d_offsets, stride, &set);
  if (rc) return rc;
  struct Range { const void *p; size_t bytes; };
  const size_t N = (size_t)nframes, span = d_offsets ? 0 : N * (size_t)stride;
  const Range outs[6] = {{d_sel, 4 * N * top}, {d_sel_counts, 4 * N}, {d_votes, 4 * N * N},
                         {d_pairs, 8 * (size_t)max_pairs}, {d_pair_votes, 4 * (size_t)max_pairs}, {d_summary, 32}};
  const Range ins[4] = {{d_recs, span ? span * MISIFT_POINT_BYTES : 1}, {d_q, span ? span * 128 : 1}, {d_counts, 4 * N},
                        {d_offsets, d_offsets ? 4 * N : 0}};
  const auto overlap = [](const Range &a, const Range &b) {
    const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
    return a.bytes && b.bytes && pa < pb + b.bytes && pb < pa + a.bytes;
  };
  for (int i = 0; i < 6; i++) {
    for (int j = i + 1; j < 6; j++) ARG_CHECK(!overlap(outs[i], outs[j]));
    for (int j = 0; j < 4; j++) ARG_CHECK(!overlap(outs[i], ins[j]));
  }
  RoctxRange range(__func__);
  return run_batch(ctx, {}, 0, [&](int *, void *) {
    return launch_select_pairs_batch(ctx, set, d_q, nframes, top, min_score, max_ambiguity, min_votes, k, max_pairs,
                                     d_sel, d_sel_counts, d_votes, d_pairs, d_pair_votes, d_summary);
  });
}

// The pair poses of misift_recover_pose_batch joined into one frame: a relative scale per link, the scales propagated
// from a seed pair, a camera per image along a walk.  The three host lists go to the pinned slot: links, pairs, walk.
extern "C" int misift_link_poses_batch(misift_ctx *ctx, int npairs, const int *pairs, int nimages, const void *d_rows,
                                       const int *d_row_counts, int max_pts, float min_score, float max_ambiguity,
                                       float max_error, const float *d_pose, const int *d_num_front, const float *d_xyz,
                                       int nlinks, const int *links, int seed_pair, int root_image, int min_common,
                                       int nwalk, const int *walk, float *d_link_ratio, int *d_link_common,
                                       float *d_pair_scale, float *d_cam, int *d_cam_pair, int *d_summary)
{
  ARG_CHECK(ctx && npairs >= 0 && nimages >= 1 && nlinks >= 0 && nwalk >= 0);
  ARG_CHECK(root_image >= 0 && root_image < nimages && min_common >= 1 && max_pts >= 1);
  ARG_CHECK(d_pair_scale && d_cam && d_cam_pair && d_summary);
  ARG_CHECK(nlinks == 0 || (links && d_link_ratio && d_link_common));
  ARG_CHECK(nwalk == 0 || walk);
  ARG_CHECK(npairs == 0 || (pairs && d_rows && d_row_counts && d_pose && d_num_front && d_xyz));
  ARG_CHECK(npairs == 0 || (seed_pair >= 0 && seed_pair < npairs));
  ARG_CHECK(min_score == min_score && max_ambiguity == max_ambiguity);      // not NaN
  ARG_CHECK(max_error > 0.0f);                                              // NaN fails too
  for (int i = 0; i < 2 * npairs; i++) ARG_CHECK(pairs[i] >= 0 && pairs[i] < nimages);
  for (int l = 0; l < nlinks; l++) {
    const int p = links[3 * l], q = links[3 * l + 1], kind = links[3 * l + 2];
    ARG_CHECK(p >= 0 && p < npairs && q >= 0 && q < npairs && (kind == 0 || kind == 1));
    ARG_CHECK(kind == 0 ? pairs[2 * p + 1] == pairs[2 * q] : pairs[2 * p] == pairs[2 * q]);
  }
  for (int w = 0; w < nwalk; w++) ARG_CHECK(walk[w] >= 0 && walk[w] < npairs);
  RoctxRange range(__func__);
  static const int none[1] = {0};                                           // an empty list's slot is never read
  return run_batch(ctx, {HostList{nlinks ? links : none, sizeof(int) * 3 * (size_t)nlinks},
                         HostList{npairs ? pairs : none, sizeof(int) * 2 * (size_t)npairs},
                         HostList{nwalk ? walk : none, sizeof(int) * (size_t)nwalk}, HostList{none, sizeof(none)}},
                   0, [&](int *h_lists, void *) {
                     return launch_link_poses_batch(ctx, npairs, nimages, nlinks, nwalk, h_lists, d_rows, d_row_counts,
                                                    max_pts, min_score, max_ambiguity, max_error, d_pose, d_num_front,
                                                    d_xyz, seed_pair, root_image, min_common, d_link_ratio,
                                                    d_link_common, d_pair_scale, d_cam, d_cam_pair, d_summary);
                   });
}

// The labels misift_link_tracks_batch wrote, turned into a compact array of tracks with their observations stored
// contiguously: select and number the roots, prefix-sum their lengths, scatter the members in index order.  All on the
// context stream, no host read.
extern "C" int misift_export_tracks_batch(misift_ctx *ctx, const void *d_recs, int nframes, const int *d_counts,
                                          const int *d_offsets, int stride, int max_records, const int *d_track,
                                          const int *d_track_len, const int *d_track_frames, int min_len,
                                          int consistent_only, int max_tracks, int max_obs, int *d_track_offsets,
                                          int *d_track_root, misift_track_obs *d_obs, int *d_record_obs, int *d_summary)
{
  ARG_CHECK(ctx && nframes >= 0);
  ARG_CHECK(d_recs && d_counts && d_track && d_track_len && d_track_frames);
  ARG_CHECK(d_track_offsets && d_track_root && d_obs && d_summary);
  ARG_CHECK(((uintptr_t)d_obs & 15) == 0);
  ARG_CHECK(max_records >= 1 && min_len >= 1 && max_tracks >= 1 && max_obs >= 1);
  ARG_CHECK(consistent_only == 0 || consistent_only == 1);
  BatchLayout set;
  int rc = batch_layout(__func__, d_recs, d_counts, d_offsets, stride, &set);
  if (rc) return rc;
  ARG_CHECK(!d_record_obs || (d_record_obs != d_track && d_record_obs != d_track_len && d_record_obs != d_track_frames));
  RoctxRange range(__func__);
  return run_batch(ctx, {}, 0, [&](int *, void *) {
    return launch_export_tracks_batch(ctx, set, nframes, max_records, d_track, d_track_len, d_track_frames, min_len,
                                      consistent_only, max_tracks, max_obs, d_track_offsets, d_track_root, d_obs,
                                      d_record_obs, d_summary);
  });
}

// ---- the track chain: the five calls over one scene
// The scene checked and filled in (TrackScene, triangulate_core.hpp): the sizes, the pointers every one of the calls
// needs, d_obs aligned for the kernels' one 16-byte load (track_obs_load) and usable intrinsics for every image.  What
// only some calls need (the points, the cameras) is taken as given and checked by the call.  S->intrinsics is the
// caller's list until the launch lambda puts the pinned copy in its place.
static int check_scene(const char *who, TrackScene *S, int max_tracks, int max_obs, const int *d_track_offsets,
                       const misift_track_obs *d_obs, const int *d_export_summary, const float *d_points,
                       const int *d_point_status, int nimages, const float *d_cam, const int *d_cam_pair,
                       const float *intrinsics)
{
  ARG_CHECK_IN(who, max_tracks >= 1 && max_obs >= 1 && nimages >= 1);
  ARG_CHECK_IN(who, d_track_offsets && d_obs && d_export_summary && intrinsics);
  ARG_CHECK_IN(who, ((uintptr_t)d_obs & 15) == 0);
  for (int i = 0; i < nimages; i++) ARG_CHECK_IN(who, intrinsics_usable(intrinsics + 4 * (size_t)i, 1));
  *S = TrackScene{max_tracks, max_obs, nimages, d_track_offsets, reinterpret_cast<const TrackObs *>(d_obs),
                  d_export_summary, d_points, d_point_status, d_cam, d_cam_pair, intrinsics};
  return MISIFT_OK;
}

// an output may be its input in place, or share no byte with it
static bool same_or_disjoint(const void *a, const void *b, size_t bytes)
{
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa == pb || pa + bytes <= pb || pb + bytes <= pa;
}

// a flag per image from a list of images, each checked to lie in [0, nimages)
static std::vector<int> held_flags(int nimages, int nhold, const int *hold)
{
  std::vector<int> held(nimages, 0);
  for (int j = 0; j < nhold; j++) held[hold[j]] = 1;
  return held;
}

// One world point per exported track under the cameras of misift_link_poses_batch: the call that joins the track chain
// to the pose chain.  The intrinsics go to the pinned slot.
extern "C" int misift_triangulate_tracks_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                               const misift_track_obs *d_obs, const int *d_export_summary, int nimages,
                                               const float *d_cam, const int *d_cam_pair, const float *intrinsics,
                                               int min_views, int num_loops, float *d_points, int *d_point_views,
                                               int *d_point_status, float *d_obs_error, int *d_summary)
{
  ARG_CHECK(ctx != nullptr);
  TrackScene S;
  int rc = check_scene(__func__, &S, max_tracks, max_obs, d_track_offsets, d_obs, d_export_summary, nullptr, nullptr,
                       nimages, d_cam, d_cam_pair, intrinsics);
  if (rc) return rc;
  ARG_CHECK(d_cam && d_cam_pair && d_points && d_point_views && d_point_status && d_summary);
  ARG_CHECK(min_views >= 2 && num_loops >= 0);
  RoctxRange range(__func__);
  return run_batch(ctx, {{intrinsics, sizeof(float) * 4 * (size_t)nimages}}, 0, [&](int *h_lists, void *) {
    S.intrinsics = reinterpret_cast<const float *>(h_lists);
    return launch_triangulate_tracks_batch(ctx, S, min_views, num_loops, d_points, d_point_views, d_point_status,
                                           d_obs_error, d_summary);
  });
}

// Every linked camera moved to minimise the reprojection error of its image's observations of the triangulated points:
// the other half of misift_triangulate_tracks_batch's minimisation.  The intrinsics and a flag per image (1 = held) go
// to the pinned slot.
extern "C" int misift_refine_cameras_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                           const misift_track_obs *d_obs, const int *d_export_summary,
                                           const float *d_points, const int *d_point_status, int nimages,
                                           const float *d_cam, const int *d_cam_pair, const float *intrinsics, int nhold,
                                           const int *hold, int min_obs, int num_loops, float max_error,
                                           int orthonormalise, float *d_cam_out, int *d_cam_obs, float *d_cam_rms,
                                           int *d_cam_steps, int *d_cam_status, int *d_summary)
{
  ARG_CHECK(ctx != nullptr);
  TrackScene S;
  int rc = check_scene(__func__, &S, max_tracks, max_obs, d_track_offsets, d_obs, d_export_summary, d_points,
                       d_point_status, nimages, d_cam, d_cam_pair, intrinsics);
  if (rc) return rc;
  ARG_CHECK(d_points && d_point_status && d_cam && d_cam_pair);
  ARG_CHECK(d_cam_out && d_cam_obs && d_cam_rms && d_cam_steps && d_cam_status && d_summary);
  ARG_CHECK(min_obs >= 3 && num_loops >= 0);
  ARG_CHECK(max_error > 0.0f);                                              // NaN fails too
  ARG_CHECK(orthonormalise == 0 || orthonormalise == 1);
  ARG_CHECK(nhold >= 0 && (nhold == 0 || hold));
  for (int j = 0; j < nhold; j++) ARG_CHECK(hold[j] >= 0 && hold[j] < nimages);
  ARG_CHECK(same_or_disjoint(d_cam, d_cam_out, sizeof(float) * 12 * (size_t)nimages));
  const std::vector<int> held = held_flags(nimages, nhold, hold);
  const float thresh2 = max_error * max_error;                              // rounded once, here
  RoctxRange range(__func__);
  return run_batch(ctx, {{intrinsics, sizeof(float) * 4 * (size_t)nimages}, {held.data(), sizeof(int) * (size_t)nimages}},
                   0, [&](int *h_lists, void *) {
                     S.intrinsics = reinterpret_cast<const float *>(h_lists);
                     return launch_refine_cameras_batch(ctx, S, h_lists + 4 * (size_t)nimages, min_obs, num_loops, thresh2,
                                                        orthonormalise, d_cam_out, d_cam_obs, d_cam_rms, d_cam_steps,
                                                        d_cam_status, d_summary);
                   });
}

// The camera of each selected image straight from its observations of the triangulated points, by batch RANSAC over
// six-point solves: for the images the walk of misift_link_poses_batch did not reach, or as a second opinion.  The
// intrinsics, the images and the seeds go to the pinned slot, in that order.
extern "C" int misift_resect_cameras_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                           const misift_track_obs *d_obs, const int *d_export_summary,
                                           const float *d_points, const int *d_point_status, int nimages,
                                           const float *intrinsics, int nsel, const int *images, const unsigned *seeds,
                                           int max_cand, int num_loops, float thresh, int min_inliers, int only_unset,
                                           int install, float *d_cam, int *d_cam_pair, float *d_res_cam, int *d_res_cand,
                                           int *d_res_inliers, int *d_res_status, int *d_summary)
{
  ARG_CHECK(ctx != nullptr);
  TrackScene S;
  int rc = check_scene(__func__, &S, max_tracks, max_obs, d_track_offsets, d_obs, d_export_summary, d_points,
                       d_point_status, nimages, d_cam, d_cam_pair, intrinsics);
  if (rc) return rc;
  ARG_CHECK(d_points && d_point_status);
  ARG_CHECK(d_res_cam && d_res_cand && d_res_inliers && d_res_status && d_summary);
  ARG_CHECK(nsel >= 0 && (nsel == 0 || (images && seeds)));
  ARG_CHECK(max_cand >= 6 && num_loops >= 1 && min_inliers >= 6);
  ARG_CHECK(thresh > 0.0f);                                                 // NaN fails too
  ARG_CHECK((only_unset == 0 || only_unset == 1) && (install == 0 || install == 1));
  ARG_CHECK(d_cam_pair || !(only_unset || install));
  ARG_CHECK(d_cam || !install);
  rc = check_frames(__func__, nsel, images, 1, nimages, 0);
  if (rc) return rc;
  ARG_CHECK(resect_cameras_batch_one_launch(max_obs, nsel, max_cand, num_loops));
  const float thresh2 = thresh * thresh;                                    // rounded once, here
  RoctxRange range(__func__);
  return run_batch(ctx, {{intrinsics, sizeof(float) * 4 * (size_t)nimages}, {images, sizeof(int) * (size_t)nsel},
                         {seeds, sizeof(unsigned) * (size_t)nsel}},
                   0, [&](int *h_lists, void *) {
                     S.intrinsics = reinterpret_cast<const float *>(h_lists);
                     const int *h_images = h_lists + 4 * (size_t)nimages;
                     return launch_resect_cameras_batch(ctx, S, nsel, h_images,
                                                        reinterpret_cast<const unsigned *>(h_images + nsel), max_cand,
                                                        num_loops, thresh2, min_inliers, only_unset, install, d_cam,
                                                        d_cam_pair, d_res_cam, d_res_cand, d_res_inliers, d_res_status,
                                                        d_summary);
                   });
}

// ---- new frames against a reconstruction: a descriptor per point, then cameras from 2-D/3-D matches
// The arguments of misift_describe_points_batch and of its host hook checked and put into a DescribeIn and a
// DescribeOut (localize_core.hpp).  Every rule of the header's error list but the NULL context is here.
static int describe_check(const char *who, DescribeIn *in, DescribeOut *out, int max_tracks, int max_obs,
                          const int *track_offsets, const misift_track_obs *obs, const int *export_summary,
                          const float *points, const int *point_status, const void *q, int nframes, const int *counts,
                          const int *offsets, int stride, int max_records, void *scene_q, void *scene_recs,
                          int *scene_count, int *point_members, int *summary)
{
  ARG_CHECK_IN(who, max_tracks >= 1 && max_obs >= 1 && max_records >= 1 && nframes >= 0);
  ARG_CHECK_IN(who, track_offsets && obs && export_summary && points && point_status && q && counts);
  ARG_CHECK_IN(who, scene_q && scene_recs && scene_count && point_members && summary);
  ARG_CHECK_IN(who, offsets || stride >= 0);
  ARG_CHECK_IN(who, (((uintptr_t)obs | (uintptr_t)q | (uintptr_t)scene_q | (uintptr_t)scene_recs) & 15) == 0);
  {
    // the call only reads its inputs: no output may share a byte with an input or with another output
    const size_t mt = (size_t)max_tracks, mo = (size_t)max_obs, nf = (size_t)nframes;
    const struct { const void *p; size_t bytes; } span[13] = {
        {scene_q, 128 * mt}, {scene_recs, MISIFT_POINT_BYTES * mt}, {scene_count, 4}, {point_members, 4 * mt},
        {summary, 32},
        {track_offsets, 4 * (mt + 1)}, {obs, 16 * mo}, {export_summary, 32}, {points, 16 * mt}, {point_status, 4 * mt},
        {q, 128 * (size_t)max_records}, {counts, 4 * nf}, {offsets, offsets ? 4 * nf : 0}};
    for (int a = 0; a < 5; a++)
      for (int b = a + 1; b < 13; b++) {
        if (!span[a].bytes || !span[b].bytes) continue;
        const uintptr_t pa = (uintptr_t)span[a].p, pb = (uintptr_t)span[b].p;
        ARG_CHECK_IN(who, pa + span[a].bytes <= pb || pb + span[b].bytes <= pa);
      }
  }
  in->s = TrackScene{max_tracks, max_obs, 0, track_offsets, reinterpret_cast<const TrackObs *>(obs), export_summary,
                     points, point_status, nullptr, nullptr, nullptr};
  in->q = reinterpret_cast<const signed char *>(q);
  in->nframes = nframes;
  in->counts = counts; in->offsets = offsets;
  in->stride = stride; in->max_records = max_records;
  *out = DescribeOut{reinterpret_cast<signed char *>(scene_q), reinterpret_cast<uint32_t *>(scene_recs), scene_count,
                     point_members, summary};
  return MISIFT_OK;
}

// An 8-bit descriptor per track point, laid out as a one-frame record set for the int8 pair matchers.  No host lists.
extern "C" int misift_describe_points_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                            const misift_track_obs *d_obs, const int *d_export_summary,
                                            const float *d_points, const int *d_point_status, const void *d_q,
                                            int nframes, const int *d_counts, const int *d_offsets, int stride,
                                            int max_records, void *d_scene_q, void *d_scene_recs, int *d_scene_count,
                                            int *d_point_members, int *d_summary)
{
  ARG_CHECK(ctx != nullptr);
  DescribeIn in;
  DescribeOut out;
  const int rc = describe_check(__func__, &in, &out, max_tracks, max_obs, d_track_offsets, d_obs, d_export_summary,
                                d_points, d_point_status, d_q, nframes, d_counts, d_offsets, stride, max_records,
                                d_scene_q, d_scene_recs, d_scene_count, d_point_members, d_summary);
  if (rc) return rc;
  RoctxRange range(__func__);
  return run_batch(ctx, {}, 0, [&](int *, void *) { return launch_describe_points_batch(ctx, in, out); });
}

// Test-only, host-only: the whole call on host arrays by the rules the kernel compiles (localize_core.hpp).
extern "C" int misift_test_describe_points(int max_tracks, int max_obs, const int *track_offsets,
                                           const misift_track_obs *obs, const int *export_summary, const float *points,
                                           const int *point_status, const void *q, int nframes, const int *counts,
                                           const int *offsets, int stride, int max_records, void *scene_q,
                                           void *scene_recs, int *scene_count, int *point_members, int *summary)
{
  DescribeIn in;
  DescribeOut out;
  const int rc = describe_check(__func__, &in, &out, max_tracks, max_obs, track_offsets, obs, export_summary, points,
                                point_status, q, nframes, counts, offsets, stride, max_records, scene_q, scene_recs,
                                scene_count, point_members, summary);
  if (rc) return rc;
  describe_points_host(in, out);
  return MISIFT_OK;
}

// The camera of each selected image from the rows of a frame matched against the scene's points, by resect's search, and
// the inliers as a scene for misift_merge_scenes_batch.  The intrinsics, the frames, the images and the seeds go to the
// pinned slot, in that order.
extern "C" int misift_localize_frames_batch(misift_ctx *ctx, const void *d_rows, int nframes_rows, const int *d_counts,
                                            const int *d_offsets, int stride, int max_tracks,
                                            const int *d_export_summary, const float *d_points,
                                            const int *d_point_status, int nimages, const float *intrinsics, int nsel,
                                            const int *frames, const int *images, const unsigned *seeds, int max_pts,
                                            float min_score, float max_ambiguity, int num_loops, float thresh,
                                            int min_inliers, int only_unset, int install, float *d_cam, int *d_cam_pair,
                                            float *d_res_cam, int *d_res_cand, int *d_res_inliers, int *d_res_status,
                                            int *d_summary, int max_found, int *d_found_offsets,
                                            misift_track_obs *d_found_obs, int *d_found_summary, float *d_found_points,
                                            int *d_found_views, int *d_found_status, int *d_found_map)
{
  ARG_CHECK(ctx != nullptr);
  ARG_CHECK(max_tracks >= 1 && nimages >= 1 && nframes_rows >= 1 && max_pts >= 1 && max_found >= 1);
  ARG_CHECK(d_rows && d_counts && d_export_summary && d_points && d_point_status && intrinsics);
  ARG_CHECK(d_res_cam && d_res_cand && d_res_inliers && d_res_status && d_summary);
  ARG_CHECK(d_found_offsets && d_found_obs && d_found_summary && d_found_points && d_found_views && d_found_status &&
            d_found_map);
  ARG_CHECK(((uintptr_t)d_found_obs & 15) == 0);
  for (int i = 0; i < nimages; i++) ARG_CHECK(intrinsics_usable(intrinsics + 4 * (size_t)i, 1));
  BatchLayout rows;
  int rc = batch_layout(__func__, d_rows, d_counts, d_offsets, stride, &rows);
  if (rc) return rc;
  ARG_CHECK(nsel >= 0 && (nsel == 0 || (frames && images && seeds)));
  ARG_CHECK(num_loops >= 1 && min_inliers >= 6);
  ARG_CHECK(min_score == min_score && max_ambiguity == max_ambiguity);      // not NaN
  ARG_CHECK(thresh > 0.0f);                                                 // NaN fails too
  ARG_CHECK((only_unset == 0 || only_unset == 1) && (install == 0 || install == 1));
  ARG_CHECK(d_cam_pair || !(only_unset || install));
  ARG_CHECK(d_cam || !install);
  rc = check_frames(__func__, nsel, frames, 1, nframes_rows, 0);
  if (!rc) rc = check_frames(__func__, nsel, images, 1, nimages, 0);
  if (rc) return rc;
  ARG_CHECK(localize_frames_batch_one_launch(nsel, max_pts, num_loops));
  TrackScene S{max_tracks, 0, nimages, nullptr, nullptr, d_export_summary, d_points, d_point_status, d_cam, d_cam_pair,
               intrinsics};
  LocalizeCall call{};
  call.nsel = nsel;
  call.rows = rows;
  call.max_pts = max_pts;
  call.min_score = min_score; call.max_ambiguity = max_ambiguity;
  call.num_loops = num_loops;
  call.thresh2 = thresh * thresh;                                           // rounded once, here
  call.min_inliers = min_inliers; call.only_unset = only_unset; call.install = install;
  call.d_cam = d_cam; call.d_cam_pair = d_cam_pair;
  call.d_res_cam = d_res_cam; call.d_res_cand = d_res_cand; call.d_res_inliers = d_res_inliers;
  call.d_res_status = d_res_status; call.d_summary = d_summary;
  call.max_found = max_found;
  call.d_found_offsets = d_found_offsets; call.d_found_obs = reinterpret_cast<TrackObs *>(d_found_obs);
  call.d_found_summary = d_found_summary; call.d_found_points = d_found_points; call.d_found_views = d_found_views;
  call.d_found_status = d_found_status; call.d_found_map = d_found_map;
  RoctxRange range(__func__);
  return run_batch(ctx, {{intrinsics, sizeof(float) * 4 * (size_t)nimages}, {frames, sizeof(int) * (size_t)nsel},
                         {images, sizeof(int) * (size_t)nsel}, {seeds, sizeof(unsigned) * (size_t)nsel}},
                   0, [&](int *h_lists, void *) {
                     S.intrinsics = reinterpret_cast<const float *>(h_lists);
                     call.h_frames = h_lists + 4 * (size_t)nimages;
                     call.h_images = call.h_frames + nsel;
                     call.h_seeds = reinterpret_cast<const unsigned *>(call.h_images + nsel);
                     return launch_localize_frames_batch(ctx, S, call);
                   });
}

// Test-only, host-only: the ordered candidate list of one frame of rows (localize_core.hpp): out5 gets x y X Y Z per
// candidate, out_row its row, out_track its point, *out_n their number.  Each output holds nrows entries.
extern "C" int misift_test_localize_candidates(const void *rows, int nrows, int T, const float *points,
                                               const int *point_status, float min_score, float max_ambiguity,
                                               float *out5, int *out_row, int *out_track, int *out_n)
{
  if (nrows < 0 || T < 0 || !out_n || (nrows > 0 && (!rows || !out5 || !out_row || !out_track)) ||
      (T > 0 && (!points || !point_status))) {
    misift_set_error("misift_test_localize_candidates: invalid argument");
    return MISIFT_EINVAL;
  }
  const float *r = reinterpret_cast<const float *>(rows);
  int n = 0;
  for (int i = 0; i < nrows; i++) {
    LocCandidate c;
    if (!loc_candidate(r + (size_t)i * (MISIFT_POINT_BYTES / 4), T, points, point_status, min_score, max_ambiguity, c))
      continue;
    float *o = out5 + 5 * (size_t)n;
    o[0] = c.x; o[1] = c.y; o[2] = c.X; o[3] = c.Y; o[4] = c.Z;
    out_row[n] = i;
    out_track[n] = c.t;
    n++;
  }
  *out_n = n;
  return MISIFT_OK;
}

// Which track of scene B holds the records of each track of scene A: where the d_map of misift_align_points_batch comes
// from.  No host lists.
extern "C" int misift_correspond_tracks_batch(misift_ctx *ctx, int shift, int max_records_a, const int *d_record_obs_a,
                                              int max_tracks_a, int max_obs_a, const int *d_track_offsets_a,
                                              const int *d_export_summary_a, int max_records_b,
                                              const int *d_record_obs_b, int max_tracks_b, int max_obs_b,
                                              const int *d_track_offsets_b, const int *d_export_summary_b, int *d_map,
                                              int *d_summary)
{
  ARG_CHECK(ctx != nullptr);
  ARG_CHECK(max_records_a >= 1 && max_tracks_a >= 1 && max_obs_a >= 1);
  ARG_CHECK(max_records_b >= 1 && max_tracks_b >= 1 && max_obs_b >= 1);
  ARG_CHECK(d_record_obs_a && d_track_offsets_a && d_export_summary_a);
  ARG_CHECK(d_record_obs_b && d_track_offsets_b && d_export_summary_b);
  ARG_CHECK(d_map && d_summary);
  RoctxRange range(__func__);
  return run_batch(ctx, {}, 0, [&](int *, void *) {
    return launch_correspond_tracks_batch(ctx, shift, max_records_a, d_record_obs_a, max_tracks_a, max_obs_a,
                                          d_track_offsets_a, d_export_summary_a, max_records_b, d_record_obs_b,
                                          max_tracks_b, max_obs_b, d_track_offsets_b, d_export_summary_b, d_map,
                                          d_summary);
  });
}

// Per entry the similarity transform between corresponding points of two pooled arrays, by batch RANSAC over three-point
// closed-form solves, refitted over its inliers.  The ranges and the seeds go to the pinned slot, in that order.
extern "C" int misift_align_points_batch(misift_ctx *ctx, const float *d_src, const int *d_src_status,
                                         const float *d_dst, const int *d_dst_status, const int *d_map, int nsel,
                                         const int *ranges, const unsigned *seeds, const int *d_count, int count_stride,
                                         int num_loops, float thresh, int min_inliers, int refit_loops, float *d_sim,
                                         int *d_align_cand, int *d_align_inliers, int *d_align_status, int *d_inlier,
                                         int *d_summary)
{
  ARG_CHECK(ctx != nullptr);
  ARG_CHECK(d_src && d_dst && d_map);
  ARG_CHECK(d_sim && d_align_cand && d_align_inliers && d_align_status && d_summary);
  ARG_CHECK(nsel >= 0 && (nsel == 0 || (ranges && seeds)));
  ARG_CHECK(num_loops >= 1 && min_inliers >= 3 && refit_loops >= 0);
  ARG_CHECK(thresh > 0.0f);                                                 // NaN fails too
  ARG_CHECK(!d_count || count_stride >= 0);
  int max_cap = 1;
  for (int e = 0; e < nsel; e++) {
    const int *r = ranges + 4 * (size_t)e;
    ARG_CHECK(r[0] >= 0 && r[1] >= 1 && r[2] >= 0 && r[3] >= 1);
    ARG_CHECK((long long)r[0] + r[1] <= 0x7fffffffLL && (long long)r[2] + r[3] <= 0x7fffffffLL);
    max_cap = r[1] > max_cap ? r[1] : max_cap;
  }
  if (d_inlier && nsel > 1) {                                               // d_inlier is per source point: no overlap
    std::vector<std::pair<int, int>> spans((size_t)nsel);
    for (int e = 0; e < nsel; e++) spans[e] = {ranges[4 * (size_t)e], ranges[4 * (size_t)e + 1]};
    std::sort(spans.begin(), spans.end());
    for (int e = 1; e < nsel; e++)
      ARG_CHECK((long long)spans[e - 1].first + spans[e - 1].second <= spans[e].first);
  }
  ARG_CHECK(align_points_batch_one_launch(nsel, max_cap, num_loops));
  const float thresh2 = thresh * thresh;                                    // rounded once, here
  RoctxRange range(__func__);
  return run_batch(ctx, {{ranges, sizeof(int) * 4 * (size_t)nsel}, {seeds, sizeof(unsigned) * (size_t)nsel}}, 0,
                   [&](int *h_lists, void *) {
                     return launch_align_points_batch(ctx, d_src, d_src_status, d_dst, d_dst_status, d_map, nsel, h_lists,
                                                      reinterpret_cast<const unsigned *>(h_lists + 4 * (size_t)nsel),
                                                      max_cap, d_count, count_stride, num_loops, thresh2, min_inliers,
                                                      refit_loops, d_sim, d_align_cand, d_align_inliers, d_align_status,
                                                      d_inlier, d_summary);
                   });
}

// A similarity transform applied to the points and the cameras of a scene.  No host lists.
extern "C" int misift_transform_scene_batch(misift_ctx *ctx, const float *d_sim, const int *d_sim_status, int max_tracks,
                                            const int *d_export_summary, const float *d_points,
                                            const int *d_point_status, int nimages, const float *d_cam,
                                            const int *d_cam_pair, float *d_points_out, float *d_cam_out)
{
  ARG_CHECK(ctx != nullptr);
  ARG_CHECK(max_tracks >= 1 && nimages >= 1);
  ARG_CHECK(d_sim && d_export_summary && d_points && d_point_status && d_cam && d_cam_pair && d_points_out && d_cam_out);
  ARG_CHECK(same_or_disjoint(d_points, d_points_out, sizeof(float) * 4 * (size_t)max_tracks));
  ARG_CHECK(same_or_disjoint(d_cam, d_cam_out, sizeof(float) * 12 * (size_t)nimages));
  RoctxRange range(__func__);
  return run_batch(ctx, {}, 0, [&](int *, void *) {
    return launch_transform_scene_batch(ctx, d_sim, d_sim_status, max_tracks, d_export_summary, d_points, d_point_status,
                                        nimages, d_cam, d_cam_pair, d_points_out, d_cam_out);
  });
}

// The body of the four bundle calls, each described by a BundleCall (bundle_host.hpp): the arguments checked, what they
// derive computed once (bundle_derive), the host lists pinned.  The intrinsics, the held flags and, with
// d_intrinsics_out, the groups go to the pinned slot in that order; for the radial call `radial` and `k0` (both or
// neither NULL: all zero) follow, padded with zeros.
static int adjust_bundle(const char *who, misift_ctx *ctx, const BundleCall &c)
{
  ARG_CHECK_IN(who, ctx != nullptr);
  TrackScene S;
  int rc = check_scene(who, &S, c.max_tracks, c.max_obs, c.track_offsets,
                       reinterpret_cast<const misift_track_obs *>(c.obs), c.export_summary, c.points, c.point_status,
                       c.nimages, c.cam, c.cam_pair, c.intrinsics);
  if (rc) return rc;
  ARG_CHECK_IN(who, c.points && c.point_status && c.cam && c.cam_pair);
  ARG_CHECK_IN(who, c.cam_out && c.points_out && c.cam_obs && c.cam_status && c.cam_rms && c.point_obs);
  ARG_CHECK_IN(who, c.cost && c.summary && (c.history || c.num_loops == 0));
  ARG_CHECK_IN(who, c.min_views >= 2 && c.min_obs >= 3 && c.num_loops >= 0 && c.cg_iters >= 0);
  ARG_CHECK_IN(who, c.max_error > 0.0f);                                            // NaN fails too
  ARG_CHECK_IN(who, c.lambda0 > 0.0f && c.lambda0 <= 3.402823466e+38f);
  ARG_CHECK_IN(who, c.orthonormalise == 0 || c.orthonormalise == 1);
  ARG_CHECK_IN(who, c.loss == MISIFT_LOSS_NONE || c.loss == MISIFT_LOSS_HUBER || c.loss == MISIFT_LOSS_GEMAN_MCCLURE);
  if (c.loss != MISIFT_LOSS_NONE)                                                   // not read with loss 0
    ARG_CHECK_IN(who, c.loss_scale > 0.0f && c.loss_scale <= 3.402823466e+38f);
  ARG_CHECK_IN(who, c.nhold >= 0 && (c.nhold == 0 || c.hold));
  for (int j = 0; j < c.nhold; j++) ARG_CHECK_IN(who, c.hold[j] >= 0 && c.hold[j] < c.nimages);
  ARG_CHECK_IN(who, same_or_disjoint(c.cam, c.cam_out, sizeof(float) * 12 * (size_t)c.nimages));
  ARG_CHECK_IN(who, same_or_disjoint(c.points, c.points_out, sizeof(float) * 4 * (size_t)c.max_tracks));
  ARG_CHECK_IN(who, c.ngroups >= 0 && c.ngroups <= MISIFT_MAX_FOCAL_GROUPS && (c.ngroups == 0 || c.group));
  for (int i = 0; c.ngroups > 0 && i < c.nimages; i++) ARG_CHECK_IN(who, c.group[i] >= -1 && c.group[i] < c.ngroups);
  if (c.radial_call) {
    ARG_CHECK_IN(who, (c.radial != nullptr) == (c.k0 != nullptr) && (c.radial_out || c.ngroups == 0));
    for (int g = 0; c.radial && g < c.ngroups; g++) {
      ARG_CHECK_IN(who, c.radial[g] == 0 || c.radial[g] == 1);
      ARG_CHECK_IN(who, c.k0[g] >= -3.402823466e+38f && c.k0[g] <= 3.402823466e+38f);   // NaN fails too
    }
  }
  const BundleDerived d = bundle_derive(c);
  const size_t n = (size_t)c.nimages, padded = c.radial_call ? sizeof d.rad : 0;
  RoctxRange range(who);
  return run_batch(ctx, {{c.intrinsics, sizeof(float) * 4 * n}, {d.held.data(), sizeof(int) * n},
                         {c.ngroups > 0 ? c.group : d.none.data(), c.intrinsics_out ? sizeof(int) * n : 0},
                         {d.rad, padded}, {d.k0, padded}},
                   0, [&](int *h_lists, void *) {
                     S.intrinsics = reinterpret_cast<const float *>(h_lists);
                     const int *h_held = h_lists + 4 * n, *h_rad = c.radial_call ? h_held + 2 * n : nullptr;
                     const float *h_k0 =
                         h_rad ? reinterpret_cast<const float *>(h_rad + MISIFT_MAX_RADIAL_GROUPS) : nullptr;
                     return launch_adjust_bundle_batch(ctx, S, c, d, {h_held, h_held + n, h_rad, h_k0});
                   });
}

// Levenberg-Marquardt over all free cameras and all active track points at once, the points eliminated in every step:
// what misift_refine_cameras_batch and misift_triangulate_tracks_batch do in turns, done jointly, under a loss (0: the
// plain sum of squares).  The intrinsics and a flag per image (1 = held) go to the pinned slot.
extern "C" int misift_adjust_bundle_robust_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                                 const misift_track_obs *d_obs, const int *d_export_summary,
                                                 const float *d_points, const int *d_point_status, int nimages,
                                                 const float *d_cam, const int *d_cam_pair, const float *intrinsics,
                                                 int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                                                 int cg_iters, float max_error, float lambda0, int orthonormalise,
                                                 int loss, float loss_scale, float *d_cam_out, float *d_points_out,
                                                 int *d_cam_obs, int *d_cam_status, float *d_cam_rms, int *d_point_obs,
                                                 float *d_history, float *d_cost, float *d_obs_weight, int *d_summary)
{
  return adjust_bundle(
      __func__, ctx,
      {.max_tracks = max_tracks, .max_obs = max_obs, .track_offsets = d_track_offsets,
       .obs = reinterpret_cast<const TrackObs *>(d_obs), .export_summary = d_export_summary, .points = d_points,
       .point_status = d_point_status, .nimages = nimages, .cam = d_cam, .cam_pair = d_cam_pair, .intrinsics = intrinsics,
       .nhold = nhold, .hold = hold, .min_views = min_views, .min_obs = min_obs, .num_loops = num_loops,
       .cg_iters = cg_iters, .max_error = max_error, .lambda0 = lambda0, .orthonormalise = orthonormalise, .loss = loss,
       .loss_scale = loss_scale, .cam_out = d_cam_out, .points_out = d_points_out, .cam_obs = d_cam_obs,
       .cam_status = d_cam_status, .cam_rms = d_cam_rms, .point_obs = d_point_obs, .history = d_history, .cost = d_cost,
       .obs_weight = d_obs_weight, .summary = d_summary});
}

// The robust call with one focal scale per camera group among the unknowns; the group of every image goes to the pinned
// slot behind the held flags.
extern "C" int misift_adjust_bundle_focal_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                                const misift_track_obs *d_obs, const int *d_export_summary,
                                                const float *d_points, const int *d_point_status, int nimages,
                                                const float *d_cam, const int *d_cam_pair, const float *intrinsics,
                                                int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                                                int cg_iters, float max_error, float lambda0, int orthonormalise,
                                                int loss, float loss_scale, int ngroups, const int *group,
                                                float *d_cam_out, float *d_points_out, int *d_cam_obs, int *d_cam_status,
                                                float *d_cam_rms, int *d_point_obs, float *d_history, float *d_cost,
                                                float *d_obs_weight, int *d_summary, float *d_intrinsics_out,
                                                int *d_focal)
{
  ARG_CHECK(d_intrinsics_out && (d_focal || ngroups == 0));
  return adjust_bundle(
      __func__, ctx,
      {.max_tracks = max_tracks, .max_obs = max_obs, .track_offsets = d_track_offsets,
       .obs = reinterpret_cast<const TrackObs *>(d_obs), .export_summary = d_export_summary, .points = d_points,
       .point_status = d_point_status, .nimages = nimages, .cam = d_cam, .cam_pair = d_cam_pair, .intrinsics = intrinsics,
       .nhold = nhold, .hold = hold, .min_views = min_views, .min_obs = min_obs, .num_loops = num_loops,
       .cg_iters = cg_iters, .max_error = max_error, .lambda0 = lambda0, .orthonormalise = orthonormalise, .loss = loss,
       .loss_scale = loss_scale, .ngroups = ngroups, .group = group, .cam_out = d_cam_out, .points_out = d_points_out,
       .cam_obs = d_cam_obs, .cam_status = d_cam_status, .cam_rms = d_cam_rms, .point_obs = d_point_obs,
       .history = d_history, .cost = d_cost, .obs_weight = d_obs_weight, .summary = d_summary,
       .intrinsics_out = d_intrinsics_out, .focal_out = d_focal});
}

// The focal call with one radial coefficient per camera group among the unknowns (applied to the observation).
extern "C" int misift_adjust_bundle_radial_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                                 const misift_track_obs *d_obs, const int *d_export_summary,
                                                 const float *d_points, const int *d_point_status, int nimages,
                                                 const float *d_cam, const int *d_cam_pair, const float *intrinsics,
                                                 int nhold, const int *hold, int min_views, int min_obs, int num_loops,
                                                 int cg_iters, float max_error, float lambda0, int orthonormalise,
                                                 int loss, float loss_scale, int ngroups, const int *group,
                                                 const int *radial, const float *k0, float *d_cam_out,
                                                 float *d_points_out, int *d_cam_obs, int *d_cam_status, float *d_cam_rms,
                                                 int *d_point_obs, float *d_history, float *d_cost, float *d_obs_weight,
                                                 int *d_summary, float *d_intrinsics_out, int *d_focal, float *d_radial)
{
  ARG_CHECK(d_intrinsics_out && (d_focal || ngroups == 0));
  return adjust_bundle(
      __func__, ctx,
      {.max_tracks = max_tracks, .max_obs = max_obs, .track_offsets = d_track_offsets,
       .obs = reinterpret_cast<const TrackObs *>(d_obs), .export_summary = d_export_summary, .points = d_points,
       .point_status = d_point_status, .nimages = nimages, .cam = d_cam, .cam_pair = d_cam_pair, .intrinsics = intrinsics,
       .nhold = nhold, .hold = hold, .min_views = min_views, .min_obs = min_obs, .num_loops = num_loops,
       .cg_iters = cg_iters, .max_error = max_error, .lambda0 = lambda0, .orthonormalise = orthonormalise, .loss = loss,
       .loss_scale = loss_scale, .ngroups = ngroups, .group = group, .radial_call = true, .radial = radial, .k0 = k0,
       .cam_out = d_cam_out, .points_out = d_points_out, .cam_obs = d_cam_obs, .cam_status = d_cam_status,
       .cam_rms = d_cam_rms, .point_obs = d_point_obs, .history = d_history, .cost = d_cost, .obs_weight = d_obs_weight,
       .summary = d_summary, .intrinsics_out = d_intrinsics_out, .focal_out = d_focal,
       .radial_out = reinterpret_cast<int *>(d_radial)});
}

// An observation list undistorted under the coefficients the radial call left on the device: one launch.  The given
// intrinsics and the groups go to the pinned slot.
extern "C" int misift_undistort_obs_batch(misift_ctx *ctx, int max_obs, const misift_track_obs *d_obs,
                                          const int *d_export_summary, int nimages, const float *intrinsics, int ngroups,
                                          const int *group, const float *d_radial, misift_track_obs *d_obs_out)
{
  ARG_CHECK(ctx != nullptr);
  ARG_CHECK(max_obs >= 1 && nimages >= 1 && d_obs && d_export_summary && intrinsics && d_obs_out);
  ARG_CHECK(((uintptr_t)d_obs & 15) == 0 && ((uintptr_t)d_obs_out & 15) == 0);
  ARG_CHECK(same_or_disjoint(d_obs, d_obs_out, sizeof(misift_track_obs) * (size_t)max_obs));
  ARG_CHECK(ngroups >= 0 && ngroups <= MISIFT_MAX_RADIAL_GROUPS && (ngroups == 0 || (group && d_radial)));
  for (int i = 0; i < nimages; i++) ARG_CHECK(intrinsics_usable(intrinsics + 4 * (size_t)i, 1));
  for (int i = 0; ngroups > 0 && i < nimages; i++) ARG_CHECK(group[i] >= -1 && group[i] < ngroups);
  const std::vector<int> none(ngroups == 0 ? nimages : 0, -1);
  RoctxRange range(__func__);
  return run_batch(ctx, {{intrinsics, sizeof(float) * 4 * (size_t)nimages},
                         {ngroups > 0 ? group : none.data(), sizeof(int) * (size_t)nimages}},
                   0, [&](int *h_lists, void *) {
                     return launch_undistort_obs_batch(ctx, max_obs, reinterpret_cast<const TrackObs *>(d_obs),
                                                       d_export_summary, nimages, reinterpret_cast<const float *>(h_lists),
                                                       h_lists + 4 * (size_t)nimages,
                                                       reinterpret_cast<const int *>(d_radial),
                                                       reinterpret_cast<TrackObs *>(d_obs_out));
                   });
}

// The plain sum of squares: loss 0 and no weights.
extern "C" int misift_adjust_bundle_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                          const misift_track_obs *d_obs, const int *d_export_summary,
                                          const float *d_points, const int *d_point_status, int nimages,
                                          const float *d_cam, const int *d_cam_pair, const float *intrinsics, int nhold,
                                          const int *hold, int min_views, int min_obs, int num_loops, int cg_iters,
                                          float max_error, float lambda0, int orthonormalise, float *d_cam_out,
                                          float *d_points_out, int *d_cam_obs, int *d_cam_status, float *d_cam_rms,
                                          int *d_point_obs, float *d_history, float *d_cost, int *d_summary)
{
  return misift_adjust_bundle_robust_batch(ctx, max_tracks, max_obs, d_track_offsets, d_obs, d_export_summary, d_points,
                                           d_point_status, nimages, d_cam, d_cam_pair, intrinsics, nhold, hold, min_views,
                                           min_obs, num_loops, cg_iters, max_error, lambda0, orthonormalise,
                                           MISIFT_LOSS_NONE, 0.0f, d_cam_out, d_points_out, d_cam_obs, d_cam_status,
                                           d_cam_rms, d_point_obs, d_history, d_cost, nullptr, d_summary);
}

// The observation lists gated against the current points and cameras and written out again in export's format: per
// slot the reprojection gate, per track the duplicate frames, the view count and the widest angle.  The intrinsics go to
// the pinned slot.
extern "C" int misift_filter_tracks_batch(misift_ctx *ctx, int max_tracks, int max_obs, const int *d_track_offsets,
                                          const misift_track_obs *d_obs, const int *d_export_summary,
                                          const float *d_points, const int *d_point_status, int nimages,
                                          const float *d_cam, const int *d_cam_pair, const float *intrinsics,
                                          float max_error, float max_cos, int min_views, int unique_frames,
                                          int *d_track_offsets_out, misift_track_obs *d_obs_out,
                                          int *d_export_summary_out, float *d_points_out, int *d_point_views_out,
                                          int *d_point_status_out, int *d_track_map, int *d_obs_map, int *d_summary)
{
  ARG_CHECK(ctx != nullptr);
  TrackScene S;
  int rc = check_scene(__func__, &S, max_tracks, max_obs, d_track_offsets, d_obs, d_export_summary, d_points,
                       d_point_status, nimages, d_cam, d_cam_pair, intrinsics);
  if (rc) return rc;
  ARG_CHECK(d_points && d_point_status && d_cam && d_cam_pair);
  ARG_CHECK(d_track_offsets_out && d_obs_out && d_export_summary_out && d_points_out);
  ARG_CHECK(d_point_views_out && d_point_status_out && d_track_map && d_summary);
  ARG_CHECK(((uintptr_t)d_obs_out & 15) == 0);
  ARG_CHECK(min_views >= 2 && (unique_frames == 0 || unique_frames == 1));
  ARG_CHECK(max_error > 0.0f);                                              // NaN fails too
  ARG_CHECK(max_cos == max_cos);
  {
    // compaction moves entries across workgroups: no output may share a byte with an input or with another output
    const size_t mt = (size_t)max_tracks, mo = (size_t)max_obs, n = (size_t)nimages;
    const struct { const void *p; size_t bytes; } span[16] = {
        {d_track_offsets_out, 4 * (mt + 1)}, {d_obs_out, 16 * mo}, {d_export_summary_out, 32}, {d_points_out, 16 * mt},
        {d_point_views_out, 4 * mt}, {d_point_status_out, 4 * mt}, {d_track_map, 4 * mt}, {d_obs_map, 4 * mo},
        {d_summary, 32},
        {d_track_offsets, 4 * (mt + 1)}, {d_obs, 16 * mo}, {d_export_summary, 32}, {d_points, 16 * mt},
        {d_point_status, 4 * mt}, {d_cam, 48 * n}, {d_cam_pair, 4 * n}};
    for (int a = 0; a < 9; a++)
      for (int b = a + 1; b < 16; b++) {
        if (!span[a].p || !span[b].p) continue;                             // d_obs_map may be NULL
        const uintptr_t pa = (uintptr_t)span[a].p, pb = (uintptr_t)span[b].p;
        ARG_CHECK(pa + span[a].bytes <= pb || pb + span[b].bytes <= pa);
      }
  }
  const float thresh2 = max_error * max_error;                              // rounded once, here
  RoctxRange range(__func__);
  return run_batch(ctx, {{intrinsics, sizeof(float) * 4 * (size_t)nimages}}, 0, [&](int *h_lists, void *) {
    S.intrinsics = reinterpret_cast<const float *>(h_lists);
    return launch_filter_tracks_batch(ctx, S, thresh2, max_cos, min_views, unique_frames, d_track_offsets_out, d_obs_out,
                                      d_export_summary_out, d_points_out, d_point_views_out, d_point_status_out,
                                      d_track_map, d_obs_map, d_summary);
  });
}

// Two scenes in one gauge written out as one: the arguments of misift_merge_scenes_batch and of its host hook checked
// and put into a MergeIn (merge_core.hpp).  Every rule of the header's error list but the NULL context is here.
static int merge_check(const char *who, MergeIn *in, int max_tracks_a, int max_obs_a, const int *track_offsets_a, const misift_track_obs *obs_a,
                      const int *export_summary_a, const float *points_a, const int *point_views_a,
                      const int *point_status_a, int nimages_a, const float *cam_a, const int *cam_pair_a,
                      int max_records_a, const int *record_obs_a, int max_tracks_b, int max_obs_b,
                      const int *track_offsets_b, const misift_track_obs *obs_b, const int *export_summary_b,
                      const float *points_b, const int *point_views_b, const int *point_status_b, int nimages_b,
                      const float *cam_b, const int *cam_pair_b, int max_records_b, const int *record_obs_b,
                      const int *map, const int *accept, int fshift_a, int fshift_b, int nimages_out, int rshift_a,
                      int rshift_b, int max_records_out, int max_tracks_out, int max_obs_out, int *track_offsets_out,
                      misift_track_obs *obs_out, int *export_summary_out, float *points_out, int *point_views_out,
                      int *point_status_out, float *cam_out, int *cam_pair_out, int *track_map_a, int *obs_map_a,
                      int *obs_map_b, int *record_obs_out, int *summary)
{
  ARG_CHECK_IN(who, max_tracks_a >= 1 && max_obs_a >= 1 && nimages_a >= 1);
  ARG_CHECK_IN(who, max_tracks_b >= 1 && max_obs_b >= 1 && nimages_b >= 1);
  ARG_CHECK_IN(who, max_tracks_out >= 1 && max_obs_out >= 1 && nimages_out >= 1);
  ARG_CHECK_IN(who, track_offsets_a && obs_a && export_summary_a && points_a && point_views_a && point_status_a);
  ARG_CHECK_IN(who, track_offsets_b && obs_b && export_summary_b && points_b && point_views_b && point_status_b);
  ARG_CHECK_IN(who, cam_a && cam_pair_a && cam_b && cam_pair_b && map);
  ARG_CHECK_IN(who, track_offsets_out && obs_out && export_summary_out && points_out && point_views_out);
  ARG_CHECK_IN(who, point_status_out && cam_out && cam_pair_out && track_map_a && summary);
  ARG_CHECK_IN(who, fshift_a >= 0 && fshift_b >= 0 && rshift_a >= 0 && rshift_b >= 0);
  ARG_CHECK_IN(who, (long long)nimages_a + fshift_a <= nimages_out && (long long)nimages_b + fshift_b <= nimages_out);
  if (record_obs_out) {
    ARG_CHECK_IN(who, record_obs_a && record_obs_b);
    ARG_CHECK_IN(who, max_records_a >= 1 && max_records_b >= 1 && max_records_out >= 1);
    ARG_CHECK_IN(who, (long long)max_records_a + rshift_a <= max_records_out);
    ARG_CHECK_IN(who, (long long)max_records_b + rshift_b <= max_records_out);
  }
  ARG_CHECK_IN(who, (((uintptr_t)obs_a | (uintptr_t)obs_b | (uintptr_t)obs_out) & 15) == 0);
  {
    // the copy moves entries across workgroups: no output may share a byte with an input or with another output
    const size_t ta = (size_t)max_tracks_a, oa = (size_t)max_obs_a, na = (size_t)nimages_a;
    const size_t tb = (size_t)max_tracks_b, ob = (size_t)max_obs_b, nb = (size_t)nimages_b;
    const size_t to = (size_t)max_tracks_out, oo = (size_t)max_obs_out, no = (size_t)nimages_out;
    const size_t ra = record_obs_out ? (size_t)max_records_a : 0, rb = record_obs_out ? (size_t)max_records_b : 0;
    const struct { const void *p; size_t bytes; } span[33] = {
        {track_offsets_out, 4 * (to + 1)}, {obs_out, 16 * oo}, {export_summary_out, 32}, {points_out, 16 * to},
        {point_views_out, 4 * to}, {point_status_out, 4 * to}, {cam_out, 48 * no}, {cam_pair_out, 4 * no},
        {track_map_a, 4 * ta}, {obs_map_a, 4 * oa}, {obs_map_b, 4 * ob}, {record_obs_out, 4 * (size_t)max_records_out},
        {summary, 32},
        {track_offsets_a, 4 * (ta + 1)}, {obs_a, 16 * oa}, {export_summary_a, 32}, {points_a, 16 * ta},
        {point_views_a, 4 * ta}, {point_status_a, 4 * ta}, {cam_a, 48 * na}, {cam_pair_a, 4 * na}, {record_obs_a, 4 * ra},
        {track_offsets_b, 4 * (tb + 1)}, {obs_b, 16 * ob}, {export_summary_b, 32}, {points_b, 16 * tb},
        {point_views_b, 4 * tb}, {point_status_b, 4 * tb}, {cam_b, 48 * nb}, {cam_pair_b, 4 * nb}, {record_obs_b, 4 * rb},
        {map, 4 * ta}, {accept, 4 * ta}};
    for (int a = 0; a < 13; a++)
      for (int b = a + 1; b < 33; b++) {
        if (!span[a].p || !span[b].p || !span[a].bytes || !span[b].bytes) continue;    // the optional ones
        const uintptr_t pa = (uintptr_t)span[a].p, pb = (uintptr_t)span[b].p;
        ARG_CHECK_IN(who, pa + span[a].bytes <= pb || pb + span[b].bytes <= pa);
      }
  }
  const TrackScene sa{max_tracks_a, max_obs_a, nimages_a, track_offsets_a, reinterpret_cast<const TrackObs *>(obs_a),
                      export_summary_a, points_a, point_status_a, cam_a, cam_pair_a, nullptr};
  const TrackScene sb{max_tracks_b, max_obs_b, nimages_b, track_offsets_b, reinterpret_cast<const TrackObs *>(obs_b),
                      export_summary_b, points_b, point_status_b, cam_b, cam_pair_b, nullptr};
  in->a = MergeScene{sa, point_views_a, record_obs_out ? record_obs_a : nullptr, max_records_a, fshift_a, rshift_a};
  in->b = MergeScene{sb, point_views_b, record_obs_out ? record_obs_b : nullptr, max_records_b, fshift_b, rshift_b};
  in->map = map;
  in->accept = accept;
  in->out = MergeOut{max_tracks_out, max_obs_out, nimages_out, max_records_out, track_offsets_out,
                     reinterpret_cast<TrackObs *>(obs_out), export_summary_out, points_out, point_views_out,
                     point_status_out, cam_out, cam_pair_out, track_map_a, obs_map_a, obs_map_b, record_obs_out, summary};
  return MISIFT_OK;
}

extern "C" int misift_merge_scenes_batch(misift_ctx *ctx, int max_tracks_a, int max_obs_a, const int *track_offsets_a, const misift_track_obs *obs_a,
                      const int *export_summary_a, const float *points_a, const int *point_views_a,
                      const int *point_status_a, int nimages_a, const float *cam_a, const int *cam_pair_a,
                      int max_records_a, const int *record_obs_a, int max_tracks_b, int max_obs_b,
                      const int *track_offsets_b, const misift_track_obs *obs_b, const int *export_summary_b,
                      const float *points_b, const int *point_views_b, const int *point_status_b, int nimages_b,
                      const float *cam_b, const int *cam_pair_b, int max_records_b, const int *record_obs_b,
                      const int *map, const int *accept, int fshift_a, int fshift_b, int nimages_out, int rshift_a,
                      int rshift_b, int max_records_out, int max_tracks_out, int max_obs_out, int *track_offsets_out,
                      misift_track_obs *obs_out, int *export_summary_out, float *points_out, int *point_views_out,
                      int *point_status_out, float *cam_out, int *cam_pair_out, int *track_map_a, int *obs_map_a,
                      int *obs_map_b, int *record_obs_out, int *summary)
{
  ARG_CHECK(ctx != nullptr);
  MergeIn in;
  const int rc = merge_check(__func__, &in, max_tracks_a, max_obs_a, track_offsets_a, obs_a, export_summary_a, points_a, point_views_a, point_status_a,
                      nimages_a, cam_a, cam_pair_a, max_records_a, record_obs_a, max_tracks_b, max_obs_b, track_offsets_b,
                      obs_b, export_summary_b, points_b, point_views_b, point_status_b, nimages_b, cam_b, cam_pair_b,
                      max_records_b, record_obs_b, map, accept, fshift_a, fshift_b, nimages_out, rshift_a, rshift_b,
                      max_records_out, max_tracks_out, max_obs_out, track_offsets_out, obs_out, export_summary_out,
                      points_out, point_views_out, point_status_out, cam_out, cam_pair_out, track_map_a, obs_map_a,
                      obs_map_b, record_obs_out, summary);
  if (rc) return rc;
  RoctxRange range(__func__);
  return run_batch(ctx, {}, 0, [&](int *, void *) { return launch_merge_scenes_batch(ctx, in); });
}

// Test-only, host-only: the whole call on host arrays by the rules the kernels compile (merge_core.hpp).
extern "C" int misift_test_merge_scenes(int max_tracks_a, int max_obs_a, const int *track_offsets_a, const misift_track_obs *obs_a,
                      const int *export_summary_a, const float *points_a, const int *point_views_a,
                      const int *point_status_a, int nimages_a, const float *cam_a, const int *cam_pair_a,
                      int max_records_a, const int *record_obs_a, int max_tracks_b, int max_obs_b,
                      const int *track_offsets_b, const misift_track_obs *obs_b, const int *export_summary_b,
                      const float *points_b, const int *point_views_b, const int *point_status_b, int nimages_b,
                      const float *cam_b, const int *cam_pair_b, int max_records_b, const int *record_obs_b,
                      const int *map, const int *accept, int fshift_a, int fshift_b, int nimages_out, int rshift_a,
                      int rshift_b, int max_records_out, int max_tracks_out, int max_obs_out, int *track_offsets_out,
                      misift_track_obs *obs_out, int *export_summary_out, float *points_out, int *point_views_out,
                      int *point_status_out, float *cam_out, int *cam_pair_out, int *track_map_a, int *obs_map_a,
                      int *obs_map_b, int *record_obs_out, int *summary)
{
  MergeIn in;
  const int rc = merge_check(__func__, &in, max_tracks_a, max_obs_a, track_offsets_a, obs_a, export_summary_a, points_a, point_views_a, point_status_a,
                      nimages_a, cam_a, cam_pair_a, max_records_a, record_obs_a, max_tracks_b, max_obs_b, track_offsets_b,
                      obs_b, export_summary_b, points_b, point_views_b, point_status_b, nimages_b, cam_b, cam_pair_b,
                      max_records_b, record_obs_b, map, accept, fshift_a, fshift_b, nimages_out, rshift_a, rshift_b,
                      max_records_out, max_tracks_out, max_obs_out, track_offsets_out, obs_out, export_summary_out,
                      points_out, point_views_out, point_status_out, cam_out, cam_pair_out, track_map_a, obs_map_a,
                      obs_map_b, record_obs_out, summary);
  if (rc) return rc;
  merge_scenes_host(in);
  return MISIFT_OK;
}

// ------------------------------------------------------------------- timing
extern "C" int misift_timer_start(misift_ctx *ctx)
{
  ARG_CHECK(ctx != nullptr);
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  return MISIFT_OK;
}

extern "C" int misift_timer_stop_ms(misift_ctx *ctx, float *ms_out)
{
  ARG_CHECK(ctx && ms_out);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  HIP_TRY(hipEventElapsedTime(ms_out, ctx->ev0, ctx->ev1));
  return MISIFT_OK;
}

extern "C" int misift_profile_enable(misift_ctx *ctx, int on)
{
  ARG_CHECK(ctx != nullptr);
  int rc = resolve_profile(ctx);
  ctx->profile = on != 0;
  for (misift_ctx *l : extra(ctx)->lanes) {
    const int r2 = resolve_profile(l);
    l->profile = on != 0;
    if (!rc) rc = r2;
  }
  return rc;
}

extern "C" int misift_profile_reset(misift_ctx *ctx)
{
  ARG_CHECK(ctx != nullptr);
  int rc = resolve_profile(ctx);
  ctx->nprof = 0;
  for (misift_ctx *l : extra(ctx)->lanes) {
    const int r2 = resolve_profile(l);
    l->nprof = 0;
    if (!rc) rc = r2;
  }
  return rc;
}

extern "C" int misift_profile_read(misift_ctx *ctx, int cap, char (*names)[32], float *total_ms, int *calls, int *n_out)
{
  ARG_CHECK(ctx && names && total_ms && calls && n_out);
  int rc = resolve_profile(ctx);
  if (rc) return rc;
  int n = 0;
  // the context's own launches, then those of its pipelines (batches in flight), merged by kernel name
  std::vector<misift_ctx *> all(1, ctx);
  for (misift_ctx *l : extra(ctx)->lanes) {
    rc = resolve_profile(l);
    if (rc) return rc;
    all.push_back(l);
  }
  for (misift_ctx *c : all)
    for (int i = 0; i < c->nprof; i++) {
      int j = 0;
      while (j < n && strncmp(names[j], c->prof[i].name, 32) != 0) j++;
      if (j == n) {
        if (n == cap) continue;
        memcpy(names[n], c->prof[i].name, 32);
        total_ms[n] = 0.0f;
        calls[n] = 0;
        n++;
      }
      total_ms[j] += c->prof[i].total_ms;
      calls[j] += c->prof[i].calls;
    }
  *n_out = n;
  return MISIFT_OK;
}
