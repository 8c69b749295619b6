// Internal definitions shared by the HIP translation units of libicgvins_hip.so (gfx950 only).
#pragma once
#include <utility>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/icgvins_hip.h"

#define ICG_MAX_LEVELS 4
#define ICG_LK_WIN 21
#define ICG_LK_HALF 10
#define ICG_CLAHE_TILES 21

struct icg_level {
    int w, h, pitch;
    size_t off; // byte offset inside a slot
};

struct icg_prof_rec {
    int launches  = 0;
    double total_ms = 0;
};

// Deterministic assembly plan of a partition of the resident reprojection factors (reproj_asm.hip).  The order in which every sum of the
// normal equations is formed is a function of the window's own factor list only — not of launch geometry, batch composition or timing:
//   runs    factors of a window grouped by their ordered (reference pose, observer pose) pair, list order kept inside a run; every run
//           is reduced by one wave into the 20 x 20 block [Ji Jj Je Jtd -r]^T [Ji Jj Je Jtd -r] (k_asm_runs);
//   lrec    factors of a window grouped by landmark, list order kept; the landmark rows (G_l, h_ll, b_l) are gathered from them.
struct icg_asm_plan {
    int n_runs = 0, Kmax = 1;
    std::vector<int32_t> run_off;   // W+1: window w owns runs [run_off[w], run_off[w+1])
    std::vector<int32_t> pose_off;  // W+1 into pose_glob
    std::vector<int32_t> pose_glob; // local pose number -> global pose index (ascending inside a window)
    char *d_buf = nullptr;          // one allocation for the five index arrays below
    size_t buf_cap = 0;             // bytes
    int32_t *d_perm = nullptr;      // n: factor indices, run-major
    int32_t *d_runs = nullptr;      // n_runs x 4: first (into d_perm), count, local_i | local_j << 16, window
    int32_t *d_run_off = nullptr;   // W+1
    int32_t *d_pair_run = nullptr;  // W x Kmax^2: run of the ordered local pose pair, -1 = none
    int32_t *d_lrec = nullptr;      // n x 4: factor, local_i, local_j, 0 — landmark-major
    int32_t *d_lm_foff = nullptr;   // n_lm+1: landmark l owns d_lrec[lm_foff[l] .. lm_foff[l+1])
    double *d_part = nullptr;       // n_runs x 220: the runs' blocks (upper-triangular 2 x 2 tiles)
    size_t part_cap = 0;            // bytes
};
struct icg_partition {
    int W = 0;
    bool plan_valid = false;
    std::vector<int32_t> fac_off, lm_off; // W+1 each
    std::vector<int64_t> sys_off;         // W+1: start of window w's (H | b | inv) block inside d_sys, in doubles
    std::vector<double> damp;             // damping that went into each window's inv
    int sys_P = 0, sys_valid = 0;
    icg_asm_plan plan;
};

// What the evaluation of a resident factor set leaves on the device, and whether it may be read: the record every set below embeds, and
// the one place its protocol is written.  The buffers grow on demand and are freed with the context.  A *_set entry invalidates first
// (the old set is gone, also when the call then fails); an evaluation reserves, invalidates again behind its launch guard and ends after finish();
// every reader asks icg_resident_require.  A flag left true over a replaced buffer would let a kernel read freed memory.
struct icg_resident_results {
    double *d_res = nullptr, *d_jac = nullptr;
    size_t res_cap = 0, jac_cap = 0;           // bytes
    bool res_valid = false, jac_valid = false; // evaluated (with Jacobians) since the set was made resident
};

// Resident marginalization priors (marg.hip): everything icg_marg_prior_evaluate needs besides x.  The buffers grow on demand and are
// freed with the context; n = 0: no set is resident.
struct icg_marg_set {
    int n = 0, n_blocks = 0;
    int64_t total_r = 0, total_x = 0, total_j = 0, total_jac = 0, max_jac = 0; // elements: residuals, parameters, J0, Jacobian blocks (all / largest window)
    double *d_J = nullptr;  // 2 x total_j: J0 row-major | J0 transposed
    double *d_e0 = nullptr, *d_x0 = nullptr;
    char *d_meta = nullptr; // offsets and block layout (marg.hip marg_view)
    size_t J_cap = 0, e0_cap = 0, x0_cap = 0, meta_cap = 0; // bytes
    std::vector<int64_t> h_meta;
    icg_resident_results out; // d_res: the residuals of the last icg_marg_prior_evaluate_resident (total_r), read in place by icg_reproj_host_parts_build_prior; the Jacobian half is never reserved
    // what the host-part entry validates and places a prior block by (n entries each, written by icg_marg_prior_set beside h_meta): the
    // retained size of window w, its first residual and the first element of its J0
    std::vector<int32_t> h_r, h_e_off;
    std::vector<int64_t> h_j_off;
};

// Resident preintegration factors (preint_shared.h): everything *_evaluate_resident needs besides the evaluation points and the correction
// quaternions, in one buffer that grows on demand and is freed with the context; n = 0: no set is resident.  One type for both families, one
// member of the context each (preint: N = 15, delta 16, point 32; preint_odo: N = 19, delta 20, point 34), so a context may hold one set of
// each at once.  The results of the last evaluation stay in out.d_res (N per factor) and out.d_jac (N x point row-major per factor).
struct icg_preint_resident {
    int n = 0;
    int64_t total_pn = 0; // rows of pn
    char *d_set = nullptr; // delta_state delta n | jac NN n | sqrt_info NN n | delta_time n | env 4n | q_nn 4n | pn 4 total_pn | pn_offsets n+1 | variant n
    size_t set_cap = 0;    // bytes
    icg_resident_results out;
};

// Resident navigation factors (nav.hip): kinds, offsets and constants of the members in one buffer that grows on demand and is freed with the
// context; n = 0: no set is resident.  The results of the last evaluation stay in out.d_res (nr per member) and out.d_jac (nr x width row-major per
// member), both concatenated in member order.
struct icg_nav_resident {
    int n = 0;
    int64_t total_aux = 0;
    char *d_set = nullptr; // aux total_aux | kind n | aux_off n | r_off n+1 | j_off n+1 | p_off n+1
    size_t set_cap = 0;    // bytes
    std::vector<int32_t> h_kind, h_r_off, h_j_off, h_p_off; // host copies: widths place the points, offsets place a member for the host-part entry
    icg_resident_results out;
    bool corrected = false;                    // icg_nav_correct_resident ran on what the last evaluation kept
    bool any_robust = false;                   // a correction of this set has marked a member: the host-part gather then waits for every evaluation's correction
};
// residuals and block width of a navigation factor by kind 0..5: {3, 6, 6, 9, 7, 10} and {7, 9, 7, 9, 10, 10}, a nibble each
__host__ __device__ static inline int icg_nav_nr(int kind) { return (0xA79663 >> (4 * kind)) & 15; }
__host__ __device__ static inline int icg_nav_width(int kind) { return (0xAA9797 >> (4 * kind)) & 15; }

// The linearization icg_marg_linearize_batch_keep left on the device (marg_linearize.hip): J0 of every window (r x r row-major, window after
// window), then e0 of every window, in one buffer the context owns.  id = 0: nothing is kept.  A live id is listed in the process-wide table
// of ctx.hip (icg_kept_register / icg_kept_drop / icg_kept_lookup), through which icg_marg_prior_set_from_kept of any context finds it.
struct icg_lin_kept {
    uint64_t id = 0;
    double *d_buf = nullptr;
    size_t cap = 0; // bytes
    int64_t total_rr = 0, total_r = 0;
    std::vector<int32_t> r;             // per kept window
    std::vector<int64_t> rr_off, r_off; // its J0 in d_buf; its e0 in d_buf + total_rr
};

// Host-factor parts built on the device (host_part.hip): the Jacobian of every factor block of every window, kept densely (window after
// window, block after block) in one of two device buffers until a rebuild replaces it; a call that changes the layout moves what stays
// into the other buffer.  win is empty while nothing is kept.
struct icg_hp_block {
    int64_t off; // into d_J[cur], in doubles
    int32_t nr, nf;
};
struct icg_hp_kept {
    std::vector<std::vector<icg_hp_block>> win; // per window of the partition: its kept blocks, by position in the window's block list
    double *d_J[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0}; // bytes
    int cur = 0;
    int H_P = 0; // the P whose slots of P (P + 1) / 2 doubles the host parts in d_red_H are laid out by
};

struct icg_ctx {
    icg_ctx_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    // completion wait of a call: spin on the stream (lowest latency) or sleep on a blocking event (frees the host core for
    // other contexts' threads; ICG_WAIT_MODE=block)
    hipEvent_t ev_wait = nullptr;
    bool wait_mode_env = false;
    long poll_sleep_ns = 0; // > 0: query the stream and sleep in between (ICG_WAIT_MODE=poll[:<us>])

    // frame slots: CLAHE image + LK pyramid, u8, per-level pitch
    int n_levels = 0;
    icg_level lv[ICG_MAX_LEVELS]{};
    size_t slot_bytes = 0;
    uint8_t *d_frames = nullptr;

    // preprocessing workspace (per batch lane)
    int raw_pitch      = 0;
    uint8_t *d_raw     = nullptr; // max_batch x raw_pitch x h  gray input
    uint8_t *d_bgr     = nullptr; // lazily: max_batch x w*3 x h
    uint8_t *d_lut     = nullptr; // max_batch x tiles^2 x 256
    double *d_histmean = nullptr; // max_batch

    // detection workspace (lazily allocated)
    uint32_t *d_roi_max   = nullptr;
    unsigned long long *d_cand = nullptr;
    int32_t *d_cand_cnt   = nullptr;
    int roi_state_cap     = 0;       // entries of d_roi_max / d_cand_cnt (zero between calls: k_select clears what it consumed)
    size_t cand_cap_per_roi = 0;

    // mirrored staging arena (pinned host <-> device), bump-allocated per call
    char *h_arena = nullptr;
    char *d_arena = nullptr;
    size_t arena_cap = 0, arena_off = 0;
    size_t arena_inflight = 0; // end of the inputs staged by calls that returned without waiting (icg_call::finish_async): the next call stages behind them
    bool arena_overflow = false; // an allocation did not fit (sticky until the call's seal()/finish() reports it)

    // reprojection back-end resident state
    double *d_obs = nullptr;
    int32_t *d_fidx = nullptr; // 3 x n
    int n_factors_resident = 0, factors_cap = 0;
    double *d_rJ = nullptr; // n x 48 packed results (r2 + J46)
    int rJ_valid = 0, rJ_has_jac = 0;
    int last_n_poses = 0, last_n_lm = 0;
    double last_huber = 0.0;
    std::vector<int32_t> h_fidx; // host copy of d_fidx (3 x n): the assembly plans below are derived from it
    // pinned host memory a caller fills with a factor set before icg_reproj_commit_factors (icg_reproj_stage_factors): obs (15 x n doubles) | idx (3 x n)
    char *h_fstage = nullptr;
    size_t fstage_cap = 0;
    int fstage_n = -1;
    // f1: resident normal equations of the visual factors.  One window: H ((P+L)^2) | b | 1/(h_ll + damping) per landmark; a partition of
    // the factors into W windows (icg_reproj_set_windows) keeps one such block per window.  part_1 is the implicit partition "all resident
    // factors are one window" behind the single-window entry points — both run through the SAME kernels, so a window's sums are formed in
    // the same order alone and inside a batch.  d_sys holds the systems of whichever partition was assembled last.
    double *d_sys = nullptr;
    size_t sys_cap = 0; // bytes
    double sys_min_diag = 0.0, sys_max_diag = 0.0;
    icg_partition part_1, part_w;
    int32_t *d_fwin = nullptr;  // window of every factor (factors_cap), icg_reproj_eval_windows
    int32_t *d_lmwin = nullptr; // window of every landmark
    size_t lmwin_cap = 0; // bytes

    icg_marg_set marg;
    icg_preint_resident preint, preint_odo;
    icg_nav_resident nav;
    // M3 (marg_linearize.hip): per-window working memory of icg_marg_linearize_batch for the windows that do not fit in LDS; grows on demand
    double *d_lin_scratch = nullptr;
    size_t lin_scratch_cap = 0; // bytes
    double *d_lin_H = nullptr;  // the systems icg_marg_linearize_resident forms from the resident halves below (sum Pw^2 doubles); grows on demand
    size_t lin_H_cap = 0;       // bytes
    icg_lin_kept lin_kept;      // what icg_marg_linearize_batch_keep left for icg_marg_prior_set_from_kept
    // Reduced camera solve (chol.hip, reproj_schur.hip): the W x P x P reduced systems icg_reproj_schur_windows_resident leaves on the device, every
    // window's host-factor part (packed lower triangle, one slot of P (P + 1) / 2 doubles per window, kept until it is replaced) and the
    // working memory of the systems that do not fit in LDS; all grow on demand
    double *d_red_S = nullptr, *d_red_H = nullptr, *d_chol_scratch = nullptr;
    size_t red_S_cap = 0, red_H_cap = 0, chol_scratch_cap = 0; // bytes
    int red_P = 0, red_W = 0;                                  // shape of the resident reduced systems; red_W = 0: none
    bool red_S_valid = false;                                  // d_red_S holds the reduction of what d_sys holds now (the back-substitution reads d_sys)
    std::vector<int32_t> red_H_cols;                           // per window: columns of the resident host part, 0 = none
    icg_hp_kept hp;                                            // what icg_reproj_host_parts_build keeps to rebuild them (dropped with them)

    // every buffer icg_grow has allocated for this context: what icg_ctx_destroy frees besides the fixed allocations
    std::vector<void **> grown;

    icg_camera cam{};
    bool has_cam = false;
    // camera table (icg_set_cameras): n_cams entries resident on the device, indexed per stream by the *_cams entries; the host copy serves
    // the argument checks.  d_cams is replaced, never grown in place: a tracker copies what it needs at creation.
    icg_camera *d_cams = nullptr;
    std::vector<icg_camera> cams;

    // profiling
    bool prof_on = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    struct pending {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<pending> prof_pending;
    std::map<std::string, icg_prof_rec> prof;
};

// every window's resident host part is dropped (n_windows entries of "none"), and with them the Jacobians kept to rebuild them
static inline void icg_red_drop_host_parts(icg_ctx *ctx, size_t n_windows) {
    ctx->red_H_cols.assign(n_windows, 0);
    ctx->hp.win.clear();
}

// kept linearizations (ctx.hip): a mutex-protected process-wide table of the live ids and their contexts, so that a consumer never follows
// an id to a buffer that is gone.  register: ctx->lin_kept gets a new id (non-zero, never reused) and is listed; drop: ctx's kept set, if
// any, is unlisted and its id cleared (the buffer stays allocated for the next one); lookup: the owner of a live id, nullptr otherwise.
uint64_t icg_kept_register(icg_ctx *ctx);
void icg_kept_drop(icg_ctx *ctx);
icg_ctx *icg_kept_lookup(uint64_t id);

int icg_fail(icg_ctx *ctx, int code, const char *fmt, ...);
int icg_hip_check(icg_ctx *ctx, hipError_t e, const char *what);
#define ICG_HIP(ctx, call)                                                                                             \
    do {                                                                                                               \
        int _rc = icg_hip_check((ctx), (call), #call);                                                                 \
        if (_rc) return _rc;                                                                                           \
    } while (0)

// growable device buffers ---------------------------------------------------------------------------------
// The one way a resident device buffer grows.  *cap >= want (bytes): nothing happens.  Otherwise: wait for the context's stream (work in
// flight may still use the old buffer), free it, allocate `alloc` >= want bytes — the caller's slack policy: how often a buffer is replaced
// is part of the speed — and remember the buffer for icg_ctx_destroy.  The contents are not kept.  *replaced (if given) is set as soon as
// the old buffer is gone, also when the allocation then fails (*p = nullptr, *cap = 0): whatever the caller's state says about the old
// contents has to be invalidated on it, before the return code is looked at.
int icg_grow(icg_ctx *ctx, void **p, size_t *cap, size_t want, size_t alloc, bool *replaced = nullptr);

// resident results (icg_resident_results) ------------------------------------------------------------------
static inline void icg_resident_invalidate(icg_resident_results &o) { o.res_valid = o.jac_valid = false; }
// room for an evaluation's results, without slack (a set's size changes rarely); jac_bytes = 0: the Jacobian half is left alone.  A buffer
// that was replaced loses its flag before the return code is looked at.
static inline int icg_resident_reserve(icg_ctx *ctx, icg_resident_results &o, size_t res_bytes, size_t jac_bytes) {
    bool replaced = false;
    int rc        = icg_grow(ctx, (void **) &o.d_res, &o.res_cap, res_bytes, res_bytes, &replaced);
    if (replaced) o.res_valid = false;
    if (rc || !jac_bytes) return rc;
    replaced = false;
    rc       = icg_grow(ctx, (void **) &o.d_jac, &o.jac_cap, jac_bytes, jac_bytes, &replaced);
    if (replaced) o.jac_valid = false;
    return rc;
}
// around the kernels that write the results: behind the launch guard icg_resident_invalidate (nothing is valid until they are through),
// after finish() this
static inline void icg_resident_end(icg_resident_results &o, bool want_jac) { o.res_valid = true, o.jac_valid = want_jac; }
// The three questions every reader of a set asks, in this order, up to `need`.  n: the members of the set (0: none); the caller is the
// entry <stem><entry>, the set is made resident by <stem>_set; what: the set's noun.
enum icg_resident_need { ICG_NEED_SET, ICG_NEED_RESULTS, ICG_NEED_JACOBIANS };
static inline int icg_resident_require(icg_ctx *ctx, const icg_resident_results &o, int n, icg_resident_need need, const char *stem, const char *entry,
                                       const char *what) {
    if (n <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s%s: no %s set is resident (%s_set first)", stem, entry, what, stem);
    if (need >= ICG_NEED_RESULTS && !o.res_valid)
        return icg_fail(ctx, ICG_ERR_INVALID, "%s%s: nothing was evaluated since the set was made resident", stem, entry);
    if (need >= ICG_NEED_JACOBIANS && !o.jac_valid)
        return icg_fail(ctx, ICG_ERR_INVALID, "%s%s: the last evaluation kept no Jacobians (want_jac = 0)", stem, entry);
    return ICG_OK;
}

// large LDS --------------------------------------------------------------------------------------------------
// gfx950 has 160 KiB of LDS per CU and one workgroup may own all of it (MI355X_MICROARCH.md, "LDS"); a launch with more dynamic LDS than the
// default needs the function attribute.  The limit comes from the device the context runs on, so a build for a part with less LDS takes the
// global-memory path or reports ICG_ERR_CAPACITY instead of failing at launch.  A user whose kernel has static LDS words of its own subtracts
// them from the limit it plans with and passes on.
struct icg_lds_grant {
    std::atomic<size_t> per_dev[16]; // what the kernel was last allowed on each device; one static table per kernel
};
size_t icg_lds_limit(icg_ctx *ctx);
// before a launch of `kernel` with `bytes` of dynamic LDS: above 48 KiB, raises the kernel's attribute to `limit` (once per device)
int icg_allow_lds(icg_ctx *ctx, const void *kernel, size_t bytes, size_t limit, icg_lds_grant &granted);

// arena ---------------------------------------------------------------------------------------------------
int icg_arena_reserve(icg_ctx *ctx, size_t bytes); // ensure capacity (may reallocate; only when arena_off == 0)
static inline size_t icg_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// returns offset; host pointer = h_arena+off, device pointer = d_arena+off
size_t icg_arena_alloc(icg_ctx *ctx, size_t bytes);
template <typename T> static inline T *icg_h(icg_ctx *ctx, size_t off) { return reinterpret_cast<T *>(ctx->h_arena + off); }
template <typename T> static inline T *icg_d(icg_ctx *ctx, size_t off) { return reinterpret_cast<T *>(ctx->d_arena + off); }
int icg_arena_overflow_check(icg_ctx *ctx); // ICG_ERR_NOMEM (and the flag cleared) if an allocation since the last check did not fit
int icg_arena_h2d(icg_ctx *ctx, size_t begin, size_t end);
int icg_arena_d2h(icg_ctx *ctx, size_t begin, size_t end);
int icg_arena_drain(icg_ctx *ctx); // waits for calls that returned without waiting (arena_inflight) before the arena is reset or replaced

// profiling -----------------------------------------------------------------------------------------------
struct icg_prof_scope {
    icg_ctx *ctx;
    hipEvent_t a = nullptr, b = nullptr;
    const char *name;
    icg_prof_scope(icg_ctx *c, const char *n);
    ~icg_prof_scope();
};
void icg_prof_collect(icg_ctx *ctx); // call after stream sync

// slot helpers ---------------------------------------------------------------------------------------------
struct icg_pyr_desc { // passed by value to kernels
    uint8_t *base;    // d_frames
    unsigned long long slot_bytes;
    int n_levels;
    int w[ICG_MAX_LEVELS], h[ICG_MAX_LEVELS], pitch[ICG_MAX_LEVELS];
    unsigned int off[ICG_MAX_LEVELS];
};
icg_pyr_desc icg_make_pyr_desc(const icg_ctx *ctx);

// XCD-aware work mapping.  MI355X dispatches consecutive workgroups round-robin over its 8 XCDs, each with a private 4 MB
// L2.  Work items that share data (the LK points of one camera stream read the same two pyramids) are contiguous in the
// batch, so handing workgroup b the item  (b % 8) * ceil(n/8) + b / 8  gives every XCD one contiguous eighth of the batch
// (one stream's images per L2 instead of all of them in every L2).
// Launch 8*ceil(n/8) workgroups; items >= n exit.  A pure permutation: placement only, results unchanged.
#ifdef __HIPCC__
__device__ static inline int icg_xcd_chunked(int b, int n) { return (b & 7) * ((n + 7) >> 3) + (b >> 3); }
#endif
static inline int icg_xcd_grid(int n) { return 8 * ((n + 7) >> 3); }
// b / d for workgroup-index decoding without an integer division per thread: q = mulhi(b, ceil(2^32 / d)), exact for
// b < 2^32 / d (workgroup counts are far below that).  d = 1 has no 32-bit magic (2^32 truncates to 0, and mulhi by 0 gave quotient 0 for
// every b: a detection grid with one 60 x 64 block per ROI then decoded every block as block 0); 0 is the magic of no other divisor, so it
// stands for "the quotient is b".  Both arguments are wave-uniform where this is used: a scalar select.
static inline unsigned int icg_div_magic(int d) { return (unsigned int) ((0x100000000ull + (unsigned int) d - 1u) / (unsigned int) d); }
#ifdef __HIPCC__
__device__ static inline int icg_div_by_magic(int b, unsigned int magic) { return magic ? (int) __umulhi((unsigned int) b, magic) : b; }
#endif

#ifdef __HIPCC__
// sqrtf for x = 0 or x >= 2^-96 (no denormal argument or result): v_sqrt_f32 and the two residual tests of the compiler's own expansion of
// sqrtf — candidates r - 1 ulp, r, r + 1 ulp by the signs of the fused residuals x - c r — without the range scaling in front of it and behind
// it (5 of its 16 instructions).  Correctly rounded like the library's; the callers state why their argument is never a small non-zero value.
// (x = 0: r = 0, the pattern below it is a NaN whose test is false, the residual of the one above it is 0: the result is 0.)
__device__ static inline float icg_sqrt_unscaled(float x) {
    const float r  = __builtin_amdgcn_sqrtf(x);
    const float rm = __uint_as_float(__float_as_uint(r) - 1u), rp = __uint_as_float(__float_as_uint(r) + 1u);
    float q        = __builtin_fmaf(-rm, r, x) <= 0.f ? rm : r;
    q              = __builtin_fmaf(-rp, r, x) > 0.f ? rp : q;
    return q;
}
#endif

// single reflection, branch-free: valid for -n < i < 2n-1 (all stencil halos here overshoot by a few pixels at most)
__host__ __device__ static inline int icg_reflect1(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

__host__ __device__ static inline int icg_reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
    }
    return i;
}

int icg_stream_wait_poll(icg_ctx *ctx);
static inline int icg_stream_wait(icg_ctx *ctx) {
    if (ctx->poll_sleep_ns > 0) return icg_stream_wait_poll(ctx);
    if (ctx->ev_wait) {
        int rc = icg_hip_check(ctx, hipEventRecord(ctx->ev_wait, ctx->stream), "hipEventRecord");
        if (rc) return rc;
        return icg_hip_check(ctx, hipEventSynchronize(ctx->ev_wait), "hipEventSynchronize");
    }
    return icg_hip_check(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}

// Per-call staging helper.  The arena is pinned host memory that the GPU can address directly (hipHostMalloc), mirrored
// by a device arena at the same offsets:
//   in()/out()       mirrored: ONE H2D copy at seal(), ONE D2H copy at finish() — for data many workgroups re-read
//   in_zc()/out_zc() zero-copy: kernels read/write the pinned host memory over PCIe — for data touched once per
//                    lane/wave (point lists, status bytes); saves the copy API calls, which dominate at small batches
#define ICG_LAUNCH_GUARD(call)                \
    do {                                      \
        const int rc_guard_ = (call).outputs_done(); \
        if (rc_guard_) return rc_guard_;      \
    } while (0)

struct icg_call {
    icg_ctx *ctx;
    size_t mirror_lo = (size_t) -1, mirror_hi = 0;
    struct outrec {
        void *user;
        size_t off, bytes;
        bool zc;
    };
    std::vector<outrec> outs;
    std::vector<std::pair<size_t, size_t>> zc_regions; // [begin, end) of every zero-copy output: written by kernels through the host mapping
    explicit icg_call(icg_ctx *c) : ctx(c) { ctx->arena_off = ctx->arena_inflight; }
    int reserve(size_t bytes) {
        if (ctx->arena_inflight + bytes + 8192 <= ctx->arena_cap) return 0;
        if (int rc = icg_arena_drain(ctx)) return rc; // (growing replaces the arena: nothing may still be read from it)
        return icg_arena_reserve(ctx, bytes + 8192);
    }
    template <typename T> T *in(const T *src, size_t n) {
        size_t off = icg_arena_alloc(ctx, sizeof(T) * n);
        if (n) memcpy(ctx->h_arena + off, src, sizeof(T) * n);
        if (off < mirror_lo) mirror_lo = off;
        if (off + sizeof(T) * n > mirror_hi) mirror_hi = off + sizeof(T) * n;
        return reinterpret_cast<T *>(ctx->d_arena + off);
    }
    // a mirrored block the entry fills itself: the host pointer to write n elements through, *dev the block on the device after seal().
    // nullptr when the allocation did not fit (nothing may be written through it): the caller returns overflowed()
    template <typename T> T *stage(size_t n, T **dev) {
        const size_t off = icg_arena_alloc(ctx, sizeof(T) * n);
        if (ctx->arena_overflow) return nullptr;
        mirror_lo = std::min(mirror_lo, off), mirror_hi = std::max(mirror_hi, off + sizeof(T) * n);
        *dev = reinterpret_cast<T *>(ctx->d_arena + off);
        return reinterpret_cast<T *>(ctx->h_arena + off);
    }
    template <typename T> T *in_zc(const T *src, size_t n) {
        size_t off = icg_arena_alloc(ctx, sizeof(T) * n);
        if (n) memcpy(ctx->h_arena + off, src, sizeof(T) * n);
        return reinterpret_cast<T *>(ctx->h_arena + off);
    }
    // mirrored in-place block: uploaded at seal(), the same bytes copied back to `user` at finish() (pass user = nullptr to the
    // second argument to keep the result on the host side private: accumulators that the caller reads through another pointer)
    template <typename T> T *inout(const T *src, T *user, size_t n) {
        T *d = in(src, n);
        if (user) outs.push_back({(void *) user, (size_t) (reinterpret_cast<char *>(d) - ctx->d_arena), sizeof(T) * n, false});
        return d;
    }
    int overflowed() { return icg_arena_overflow_check(ctx); }
    // after the last in()/out()/out_zc() and BEFORE the first launch: an allocation that did not fit was redirected to offset 0, i.e. it
    // aliases the inputs staged there — no kernel may run on that (ICG_LAUNCH_GUARD returns ICG_ERR_NOMEM instead)
    int outputs_done() { return ctx->arena_overflow ? overflowed() : 0; }
    int seal() {
        if (ctx->arena_overflow) return overflowed();
        return mirror_hi > mirror_lo ? icg_arena_h2d(ctx, mirror_lo, mirror_hi) : 0;
    }
    template <typename T> T *out(T *user, size_t n) {
        size_t off = icg_arena_alloc(ctx, sizeof(T) * n);
        if (user) outs.push_back({(void *) user, off, sizeof(T) * n, false});
        return reinterpret_cast<T *>(ctx->d_arena + off);
    }
    template <typename T> T *out_zc(T *user, size_t n) {
        size_t off = icg_arena_alloc(ctx, sizeof(T) * n);
        if (user) outs.push_back({(void *) user, off, sizeof(T) * n, true});
        zc_regions.push_back({off, off + sizeof(T) * n});
        return reinterpret_cast<T *>(ctx->h_arena + off);
    }
    int finish() {
        int rc    = 0;
        if (ctx->arena_overflow) {
            (void) icg_stream_wait(ctx);
            return overflowed();
        }
        size_t lo = (size_t) -1, hi = 0;
        for (auto &o : outs)
            if (!o.zc) {
                if (o.off < lo) lo = o.off;
                if (o.off + o.bytes > hi) hi = o.off + o.bytes;
            }
        // one copy for the span of all mirrored outputs — unless a zero-copy region lies inside that span: the copy would overwrite what
        // the kernels wrote there through the host mapping with stale device-arena bytes; then every mirrored output is copied on its own
        bool spans_zc = false;
        for (auto &z : zc_regions) spans_zc |= z.first < hi && z.second > lo;
        if (hi > lo && !spans_zc) {
            rc = icg_arena_d2h(ctx, lo, hi);
        } else if (hi > lo) {
            for (auto &o : outs)
                if (!o.zc && !rc) rc = icg_arena_d2h(ctx, o.off, o.off + o.bytes);
        }
        if (rc) return rc;
        rc = icg_stream_wait(ctx);
        if (rc) return rc;
        icg_prof_collect(ctx);
        for (auto &o : outs) memcpy(o.user, ctx->h_arena + o.off, o.bytes);
        ctx->arena_off = ctx->arena_inflight = 0;
        return 0;
    }
    // A call without outputs (results stay resident: icg_reproj_eval_windows) returns as soon as its copies and kernels are enqueued — the
    // next call on the context is stream-ordered behind them and stages its inputs BEHIND this call's, which the H2D copy may still be
    // reading; the first call that waits (finish()) releases the arena.  Saves a host-device round trip per call (2 of 5 per LM step).
    int finish_async() {
        if (ctx->arena_overflow || !outs.empty() || !zc_regions.empty()) return finish();
        ctx->arena_inflight = icg_align_up(ctx->arena_off, 256);
        ctx->arena_off      = ctx->arena_inflight;
        return 0;
    }
};

// The upload of a resident set that lives in one device buffer (the *_set entries of preint_shared.h and nav.hip): *d_set grows with a
// quarter of slack, a block of `bytes` is staged for fill(char *host) to write, goes up with the call's one copy and from the arena into
// the set, device to device, under the profiler scope `scope`.  Invalidating the old set and recording the new one are the caller's.
template <typename Fill>
static inline __attribute__((always_inline)) int icg_resident_upload(icg_ctx *ctx, char **d_set, size_t *set_cap, size_t bytes, const char *scope, Fill fill) {
    int rc;
    if ((rc = icg_grow(ctx, (void **) d_set, set_cap, bytes, bytes + bytes / 4))) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(bytes + 4 * 256))) return rc;
    char *dev, *host = c.stage<char>(bytes, &dev);
    if (!host) return c.overflowed();
    fill(host);
    if ((rc = c.seal())) return rc;
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, scope);
        ICG_HIP(ctx, hipMemcpyAsync(*d_set, dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return c.finish();
}

// ---- batched Cholesky solve (chol.hip): one wave per system ---------------------------------------------------------------------------------
// A system reads its matrix as A[A_off + i * ldA + k] (k <= i), optionally + the packed host part, optionally + dd on the diagonal, in that
// order; offsets are in doubles into the arrays of icg_chol_ptrs, -1 = absent.
#define ICG_CHOL_SOLVE 1    // factor and solve (otherwise only x = 0, status = 0 and the host-part copy below)
#define ICG_CHOL_PART 2     // add the resident host part at H_off
#define ICG_CHOL_PART_NEW 4 // the host part arrives at Hnew_off: add that and store it at H_off
struct icg_chol_desc {
    int32_t n, ldA, x_len, flags; // x_len >= n: x[n .. x_len) is written as zeros
    int64_t A_off, H_off, Hnew_off, dd_off, b_off, x_off, L_off, s_off;
};
struct icg_chol_ptrs {
    const double *A, *Hnew, *dd, *b;
    double *H, *x, *L, *scratch;
    int32_t *status;
};
struct icg_chol_plan {
    int n_lds = 0, n_glob = 0, wpg = 1, lds_stride = 0; // lds_stride: doubles per wave
    std::vector<int32_t> items;                         // the systems that run in LDS first, then the others
};
// fills desc[].s_off and the plan, grows ctx->d_chol_scratch; then (after the caller staged desc and plan.items) enqueues k_chol_solve
int icg_chol_plan_build(icg_ctx *ctx, std::vector<icg_chol_desc> &desc, icg_chol_plan &plan);
int icg_chol_enqueue(icg_ctx *ctx, const icg_chol_plan &plan, const icg_chol_desc *d_desc, const int32_t *d_items, icg_chol_ptrs p);

// ---- device-resident tracker (tracker.hip): segmented / indirect launches of the primitives ----------------------------------------------
// Everything below is asynchronous on the context's stream and takes DEVICE pointers: the stage kernels of the tracker leave the work
// lists (and their lengths) in device memory, so no host round trip sizes a grid or builds a list between two stages.
struct det_roi {
    int job, block, rx, ry, rw, rh, quota, cand_base; // cand_base: offset into the job's candidate plane; quota <= 0: inactive entry
};
int icg_preprocess_launch_ind(icg_ctx *ctx, int n, const int32_t *d_slot_ind, const uint8_t *const *images, int stride, int channels, int src_on_device,
                              double *d_hist_mean);
int icg_lk_launch_segments(icg_ctx *ctx, int n_seg, int seg_cap, const int32_t *d_count, const int32_t *d_prev_slot, const int32_t *d_next_slot,
                           const float2 *d_prev, const float2 *d_guess, float2 *d_out, uint8_t *d_status, float2 *d_undist,
                           const icg_camera *d_seg_cams = nullptr); // d_seg_cams: one camera per segment (null: the context's camera)
int icg_fm_ransac_launch_sets(icg_ctx *ctx, int n_sets, int seg_cap, const int32_t *d_count, const float2 *d_p1, const float2 *d_p2, double thresh,
                              double conf, uint8_t *d_mask);
int icg_triangulate_launch_segments(icg_ctx *ctx, int n_seg, int seg_cap, const int32_t *d_count, const int32_t *d_T0, const int32_t *d_T1, int tcw_cap,
                                    const double *d_Tcw, const double *d_pc0, const double *d_pc1, double *d_pw);
int icg_detect_circle_rows(int radius, std::vector<int32_t> &vh); // vh[a] = rows of a disc column at distance a (detect.hip); -1 on failure
int icg_detect_check_grid(icg_ctx *ctx, const icg_detect_grid *grid); // ICG_ERR_INVALID for a grid the detector cannot run (detect.hip)
int icg_detect_launch_ind(icg_ctx *ctx, int n_jobs, const icg_detect_grid *grid, const void *d_rois, const int32_t *d_slots, const float2 *d_mask_pts,
                          const int32_t *d_mask_begin, const int32_t *d_mask_cnt, const int32_t *d_vh, float2 *d_picks, int32_t *d_pick_cnt,
                          float2 *d_corners, int32_t *d_corner_cnt);
