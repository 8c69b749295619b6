// Context, memory arenas and per-kernel HIP-event profiling for libicgvins_hip.so.
#include <algorithm>
#include <cstdarg>
#include <mutex>

#include <sys/prctl.h>
#include <time.h>

#include "icg_internal.h"

int icg_fail(icg_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

int icg_hip_check(icg_ctx *ctx, hipError_t e, const char *what) {
    if (e == hipSuccess) return 0;
    return icg_fail(ctx, ICG_ERR_HIP, "HIP error %d (%s) at %s", (int) e, hipGetErrorString(e), what);
}

static thread_local std::string g_create_error;

extern "C" const char *icg_version(void) { return "icgvins-hip 0.1 (gfx950)"; }

extern "C" const char *icg_last_error(const icg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

// Completion wait that does not occupy a host core: hipStreamSynchronize (and blocking events) busy-wait on this stack,
// which starves other contexts' threads when there are more contexts than cores.  Query a few times back to back (short
// kernels), then sleep between queries with a tight timer slack.
int icg_stream_wait_poll(icg_ctx *ctx) {
    static thread_local bool slack_set = false;
    if (!slack_set) {
        (void) prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
        slack_set = true;
    }
    struct timespec ts = {0, ctx->poll_sleep_ns};
    for (int it = 0;; it++) {
        hipError_t e = hipStreamQuery(ctx->stream);
        if (e == hipSuccess) return ICG_OK;
        if (e != hipErrorNotReady) return icg_hip_check(ctx, e, "hipStreamQuery");
        if (it >= 4) nanosleep(&ts, nullptr);
    }
}

extern "C" int icg_ctx_set_wait_mode(icg_ctx *ctx, int mode, int sleep_us) {
    if (!ctx || (mode != ICG_WAIT_SPIN && mode != ICG_WAIT_POLL) || (mode == ICG_WAIT_POLL && sleep_us <= 0)) return ICG_ERR_INVALID;
    if (ctx->wait_mode_env) return ICG_OK; // ICG_WAIT_MODE wins
    ctx->poll_sleep_ns = mode == ICG_WAIT_POLL ? 1000L * sleep_us : 0;
    return ICG_OK;
}

icg_pyr_desc icg_make_pyr_desc(const icg_ctx *ctx) {
    icg_pyr_desc d{};
    d.base       = ctx->d_frames;
    d.slot_bytes = ctx->slot_bytes;
    d.n_levels   = ctx->n_levels;
    for (int l = 0; l < ICG_MAX_LEVELS; l++) {
        d.w[l]     = ctx->lv[l].w;
        d.h[l]     = ctx->lv[l].h;
        d.pitch[l] = ctx->lv[l].pitch;
        d.off[l]   = (unsigned int) ctx->lv[l].off;
    }
    return d;
}

extern "C" int icg_ctx_create(const icg_ctx_config *cfg, icg_ctx **out) {
    if (!cfg || !out) return ICG_ERR_INVALID;
    *out = nullptr;
    if (cfg->width < 32 || cfg->height < 32 || cfg->n_slots < 1 || cfg->max_batch < 1 || cfg->max_points < 1) {
        g_create_error = "icg_ctx_create: invalid configuration";
        return ICG_ERR_INVALID;
    }
    // k_lk_track / k_lk_track_fb address the tiles they load from a level by ONE 32-bit byte offset per lane, row * pitch + col, formed with a
    // 24-bit multiply (lk.hip, lk_offset): every level's height and pitch stay below 2^24 and its pitch * height below 2^31.  Level 0 is the
    // largest (pitch = width rounded up to 128, as laid out below).  Checked here, before a device is touched or a byte allocated.
    if (cfg->width >= (1 << 24) || cfg->height >= (1 << 24) ||
        (unsigned long long) icg_align_up((size_t) cfg->width, 128) * (unsigned long long) cfg->height >= (1ull << 31)) {
        g_create_error = "icg_ctx_create: image too large: pitch * height of a pyramid level must stay below 2^31 bytes (32-bit tile offsets of the LK kernels)";
        return ICG_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device >= ndev) {
        g_create_error = "icg_ctx_create: no HIP device available (this library has no CPU fallback)";
        return ICG_ERR_NODEVICE;
    }
    icg_ctx *ctx = new icg_ctx();
    ctx->cfg     = *cfg;
    int rc       = 0;
    auto bail    = [&](int code) {
        g_create_error = ctx->err;
        icg_ctx_destroy(ctx);
        return code;
    };
    if ((rc = icg_hip_check(ctx, hipSetDevice(cfg->device), "hipSetDevice"))) return bail(rc);
    if ((rc = icg_hip_check(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking), "hipStreamCreate")))
        return bail(rc);

    {
        const char *wm = getenv("ICG_WAIT_MODE");
        if (wm && strncmp(wm, "poll", 4) == 0) ctx->poll_sleep_ns = (wm[4] == ':' ? atol(wm + 5) : 20) * 1000L;
        ctx->wait_mode_env = wm != nullptr;
        if (wm && strcmp(wm, "block") == 0 &&
            (rc = icg_hip_check(ctx, hipEventCreateWithFlags(&ctx->ev_wait, hipEventBlockingSync | hipEventDisableTiming), "hipEventCreate")))
            return bail(rc);
    }

    // pyramid geometry: SURVEY.md Appendix B.3 — level l is ((w+1)/2, (h+1)/2); stop when <= win.
    int w = cfg->width, h = cfg->height;
    size_t off    = 0;
    ctx->n_levels = 0;
    for (int l = 0; l < ICG_MAX_LEVELS; l++) {
        if (l > 0) {
            w = (w + 1) / 2;
            h = (h + 1) / 2;
            if (w <= ICG_LK_WIN || h <= ICG_LK_WIN) break;
        }
        ctx->lv[l].w     = w;
        ctx->lv[l].h     = h;
        ctx->lv[l].pitch = (int) icg_align_up((size_t) w, 128);
        ctx->lv[l].off   = off;
        off += icg_align_up((size_t) ctx->lv[l].pitch * h, 256);
        ctx->n_levels++;
    }
    ctx->slot_bytes = off;
    // what k_pyrdown_rows (image.hip) reads a source level with: aligned dwords, 12-byte windows that may end 8 bytes past a row
    for (int l = 0; l + 1 < ctx->n_levels; l++)
        if (ctx->lv[l].pitch % 4 != 0 || ctx->lv[l].off % 4 != 0 || ctx->lv[l].off + (size_t) ctx->lv[l].pitch * ctx->lv[l].h + 8 > ctx->slot_bytes ||
            ctx->lv[l].w < 8 || ctx->lv[l].h < 6 || ctx->lv[l].pitch < 16) {
            ctx->err = "icg_ctx_create: pyramid layout does not meet the row-stream kernel's invariants";
            return bail(ICG_ERR_INVALID);
        }
    ctx->raw_pitch  = ctx->lv[0].pitch;
    size_t tiles2   = (size_t) ICG_CLAHE_TILES * ICG_CLAHE_TILES;
    if ((rc = icg_hip_check(ctx, hipMalloc(&ctx->d_frames, ctx->slot_bytes * (size_t) cfg->n_slots), "hipMalloc frames")))
        return bail(rc);
    if ((rc = icg_hip_check(ctx, hipMalloc(&ctx->d_raw, (size_t) ctx->raw_pitch * cfg->height * cfg->max_batch),
                            "hipMalloc raw")))
        return bail(rc);
    if ((rc = icg_hip_check(ctx, hipMalloc(&ctx->d_lut, tiles2 * 256 * cfg->max_batch), "hipMalloc lut")))
        return bail(rc);
    if ((rc = icg_hip_check(ctx, hipMalloc(&ctx->d_histmean, sizeof(double) * cfg->max_batch), "hipMalloc hist")))
        return bail(rc);
    // staging arena: generous default, grows on demand
    size_t want = (size_t) cfg->max_points * 96 + (size_t) cfg->max_factors * (48 + 16) * 8 + (1u << 20);
    if ((rc = icg_arena_reserve(ctx, want))) return bail(rc);
    *out = ctx;
    return ICG_OK;
}

// ---- kept linearizations: the live ids of the process ----------------------------------------------------------
namespace {
// (never destroyed: a context may be destroyed from another library's static teardown, after this library's own)
std::mutex &g_kept_mutex          = *new std::mutex;
std::map<uint64_t, icg_ctx *> &g_kept = *new std::map<uint64_t, icg_ctx *>;
std::atomic<uint64_t> g_kept_next{1};
} // namespace

uint64_t icg_kept_register(icg_ctx *ctx) {
    const uint64_t id = g_kept_next.fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> lock(g_kept_mutex);
    g_kept[id]       = ctx;
    ctx->lin_kept.id = id;
    return id;
}

void icg_kept_drop(icg_ctx *ctx) {
    if (ctx->lin_kept.id == 0) return;
    std::lock_guard<std::mutex> lock(g_kept_mutex);
    g_kept.erase(ctx->lin_kept.id);
    ctx->lin_kept.id = 0;
}

icg_ctx *icg_kept_lookup(uint64_t id) {
    std::lock_guard<std::mutex> lock(g_kept_mutex);
    auto it = g_kept.find(id);
    return it == g_kept.end() ? nullptr : it->second;
}

extern "C" int icg_marg_linearized_release(icg_ctx *ctx) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_kept_drop(ctx);
    return ICG_OK;
}

extern "C" void icg_ctx_destroy(icg_ctx *ctx) {
    if (!ctx) return;
    icg_kept_drop(ctx); // (before its buffer is freed below)
    (void) hipSetDevice(ctx->cfg.device);
    if (ctx->stream) (void) hipStreamSynchronize(ctx->stream);
    for (auto e : ctx->ev_pool) (void) hipEventDestroy(e);
    if (ctx->ev_wait) (void) hipEventDestroy(ctx->ev_wait);
    // the front-end's fixed and lazily allocated buffers and the arena; the back-end's buffers all come from icg_grow
    void *dev[] = {ctx->d_frames, ctx->d_raw, ctx->d_bgr, ctx->d_lut, ctx->d_histmean, ctx->d_roi_max, ctx->d_cand, ctx->d_cand_cnt, ctx->d_arena, ctx->d_cams};
    for (void *p : dev)
        if (p) (void) hipFree(p);
    for (void **p : ctx->grown)
        if (*p) (void) hipFree(*p);
    if (ctx->h_arena) (void) hipHostFree(ctx->h_arena);
    if (ctx->h_fstage) (void) hipHostFree(ctx->h_fstage);
    if (ctx->stream) (void) hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int icg_ctx_sync(icg_ctx *ctx) {
    if (!ctx) return ICG_ERR_INVALID;
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icg_prof_collect(ctx);
    return ICG_OK;
}

extern "C" void *icg_ctx_stream(icg_ctx *ctx) { return ctx ? (void *) ctx->stream : nullptr; }

extern "C" int icg_set_camera(icg_ctx *ctx, const icg_camera *cam) {
    if (!ctx || !cam) return ICG_ERR_INVALID;
    ctx->cam     = *cam;
    ctx->has_cam = true;
    return ICG_OK;
}

// The camera table of the *_cams entries: one icg_camera per stream of the context, resident on the device.  The table is replaced as a
// whole (a new allocation; work queued on the stream with the old one is waited for first).
extern "C" int icg_set_cameras(icg_ctx *ctx, int n_cams, const icg_camera *cams) {
    if (!ctx) return ICG_ERR_INVALID;
    if (n_cams <= 0 || !cams) return icg_fail(ctx, ICG_ERR_INVALID, "icg_set_cameras: %d cameras, table %s", n_cams, cams ? "given" : "NULL");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_camera *d = nullptr;
    ICG_HIP(ctx, hipMalloc((void **) &d, sizeof(icg_camera) * (size_t) n_cams));
    if (icg_hip_check(ctx, hipMemcpy(d, cams, sizeof(icg_camera) * (size_t) n_cams, hipMemcpyHostToDevice), "copy camera table") ||
        icg_hip_check(ctx, hipStreamSynchronize(ctx->stream), "icg_set_cameras")) {
        (void) hipFree(d);
        return ICG_ERR_HIP;
    }
    if (ctx->d_cams) (void) hipFree(ctx->d_cams);
    ctx->d_cams = d;
    ctx->cams.assign(cams, cams + n_cams);
    return ICG_OK;
}

extern "C" int icg_pyramid_levels(const icg_ctx *ctx) { return ctx ? ctx->n_levels : 0; }

// ---- growable device buffers, large LDS --------------------------------------------------------------------
int icg_grow(icg_ctx *ctx, void **p, size_t *cap, size_t want, size_t alloc, bool *replaced) {
    if (want <= *cap) return 0;
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*p) (void) hipFree(*p);
    *p   = nullptr;
    *cap = 0;
    if (replaced) *replaced = true;
    if (std::find(ctx->grown.begin(), ctx->grown.end(), p) == ctx->grown.end()) ctx->grown.push_back(p);
    ICG_HIP(ctx, hipMalloc(p, alloc));
    *cap = alloc;
    return 0;
}

size_t icg_lds_limit(icg_ctx *ctx) {
    static std::atomic<int> per_dev[16];
    const int dev = ctx->cfg.device & 15;
    int v         = per_dev[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        int optin = 0;
        if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->cfg.device) != hipSuccess || optin <= 0) optin = 64 * 1024;
        v = optin;
        per_dev[dev].store(v, std::memory_order_relaxed);
    }
    return (size_t) v;
}

int icg_allow_lds(icg_ctx *ctx, const void *kernel, size_t bytes, size_t limit, icg_lds_grant &granted) {
    if (bytes <= 48 * 1024) return 0;
    std::atomic<size_t> &g = granted.per_dev[ctx->cfg.device & 15];
    if (g.load(std::memory_order_relaxed) >= bytes) return 0;
    ICG_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) limit));
    g.store(limit, std::memory_order_relaxed);
    return 0;
}

// ---- arena -------------------------------------------------------------------------------------------------
int icg_arena_reserve(icg_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->arena_cap) return 0;
    if (ctx->arena_off != 0) return icg_fail(ctx, ICG_ERR_NOMEM, "arena grow requested mid-call");
    size_t cap = icg_align_up(bytes + bytes / 2, 1 << 16);
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->h_arena) (void) hipHostFree(ctx->h_arena);
    if (ctx->d_arena) (void) hipFree(ctx->d_arena);
    ctx->h_arena = nullptr;
    ctx->d_arena = nullptr;
    ctx->arena_cap = 0;
    ICG_HIP(ctx, hipHostMalloc((void **) &ctx->h_arena, cap, hipHostMallocDefault));
    ICG_HIP(ctx, hipMalloc((void **) &ctx->d_arena, cap));
    ctx->arena_cap = cap;
    return 0;
}

int icg_arena_drain(icg_ctx *ctx) {
    if (ctx->arena_inflight == 0) return 0;
    int rc = icg_hip_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    ctx->arena_inflight = 0;
    ctx->arena_off      = 0;
    return rc;
}

size_t icg_arena_alloc(icg_ctx *ctx, size_t bytes) {
    size_t off = icg_align_up(ctx->arena_off, 256);
    if (off + bytes > ctx->arena_cap) {
        // the caller under-counted its reserve(): never hand out memory past the arena.  The allocation is redirected to
        // offset 0 (in bounds as long as one allocation fits) and the sticky flag fails the call at seal()/finish().
        ctx->arena_overflow = true;
        off                 = 0;
        if (bytes > ctx->arena_cap) abort(); // no in-bounds answer exists
    } else {
        ctx->arena_off = off + bytes;
    }
    return off;
}

int icg_arena_overflow_check(icg_ctx *ctx) {
    if (!ctx->arena_overflow) return 0;
    ctx->arena_overflow = false;
    ctx->arena_off      = 0;
    return icg_fail(ctx, ICG_ERR_NOMEM, "staging arena overflow: the entry point reserved too little");
}

int icg_arena_h2d(icg_ctx *ctx, size_t begin, size_t end) {
    if (end <= begin) return 0;
    ICG_HIP(ctx, hipMemcpyAsync(ctx->d_arena + begin, ctx->h_arena + begin, end - begin, hipMemcpyHostToDevice,
                                ctx->stream));
    return 0;
}
int icg_arena_d2h(icg_ctx *ctx, size_t begin, size_t end) {
    if (end <= begin) return 0;
    ICG_HIP(ctx, hipMemcpyAsync(ctx->h_arena + begin, ctx->d_arena + begin, end - begin, hipMemcpyDeviceToHost,
                                ctx->stream));
    return 0;
}

// ---- profiling ---------------------------------------------------------------------------------------------
static hipEvent_t prof_event(icg_ctx *ctx) {
    if (ctx->ev_used == ctx->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        ctx->ev_pool.push_back(e);
    }
    return ctx->ev_pool[ctx->ev_used++];
}

icg_prof_scope::icg_prof_scope(icg_ctx *c, const char *n) : ctx(c), name(n) {
    if (!ctx->prof_on) return;
    a = prof_event(ctx);
    b = prof_event(ctx);
    if (a) (void) hipEventRecord(a, ctx->stream);
}
icg_prof_scope::~icg_prof_scope() {
    if (!ctx->prof_on || !a || !b) return;
    (void) hipEventRecord(b, ctx->stream);
    ctx->prof_pending.push_back({name, a, b});
}

void icg_prof_collect(icg_ctx *ctx) {
    for (auto &p : ctx->prof_pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            auto &r = ctx->prof[p.name];
            r.launches++;
            r.total_ms += ms;
        }
    }
    ctx->prof_pending.clear();
    ctx->ev_used = 0;
}

extern "C" int icg_prof_enable(icg_ctx *ctx, int enable) {
    if (!ctx) return ICG_ERR_INVALID;
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icg_prof_collect(ctx);
    ctx->prof_on = enable != 0;
    ctx->prof.clear();
    return ICG_OK;
}

extern "C" int icg_prof_get(icg_ctx *ctx, const char *kernel_name, int *launches, double *total_ms) {
    if (!ctx || !kernel_name) return ICG_ERR_INVALID;
    auto it = ctx->prof.find(kernel_name);
    if (launches) *launches = it == ctx->prof.end() ? 0 : it->second.launches;
    if (total_ms) *total_ms = it == ctx->prof.end() ? 0.0 : it->second.total_ms;
    return ICG_OK;
}

extern "C" int icg_prof_names(icg_ctx *ctx, char *buf, int buflen) {
    if (!ctx || !buf || buflen <= 0) return ICG_ERR_INVALID;
    std::string s;
    for (auto &kv : ctx->prof) {
        s += kv.first;
        s += "\n";
    }
    snprintf(buf, (size_t) buflen, "%s", s.c_str());
    return ICG_OK;
}

// ---- raw device memory helpers -----------------------------------------------------------------------------
extern "C" int icg_dev_alloc(icg_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return ICG_ERR_INVALID;
    ICG_HIP(ctx, hipMalloc(dptr, bytes));
    return ICG_OK;
}
extern "C" int icg_dev_free(icg_ctx *ctx, void *dptr) {
    if (!ctx) return ICG_ERR_INVALID;
    ICG_HIP(ctx, hipFree(dptr));
    return ICG_OK;
}
extern "C" int icg_dev_upload(icg_ctx *ctx, void *dptr, const void *host, size_t bytes) {
    if (!ctx) return ICG_ERR_INVALID;
    ICG_HIP(ctx, hipMemcpy(dptr, host, bytes, hipMemcpyHostToDevice));
    return ICG_OK;
}
extern "C" int icg_dev_download(icg_ctx *ctx, void *host, const void *dptr, size_t bytes) {
    if (!ctx) return ICG_ERR_INVALID;
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ICG_HIP(ctx, hipMemcpy(host, dptr, bytes, hipMemcpyDeviceToHost));
    return ICG_OK;
}
