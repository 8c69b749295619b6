// Tracker core: the front-end state machine of ONE camera stream (tracking/tracking.cc:144-245 and everything it calls between the
// device primitives) as plain functions over a fixed-layout POD state, compiled TWICE from this one source:
//   * by hipcc for gfx950 (csrc/tracker.hip): the stage kernels of the device-resident tracker — the stream's rows, map points, candidate
//     lists and window live in HBM, a wave per stream runs the stage body between two device primitives, the primitives (preprocess, LK,
//     RANSAC, triangulation, detection) read their work lists where the stage body left them; the host neither builds lists nor waits
//     between stages (round 4);
//   * by g++ (host/track_table_core.cc): the same bodies behind the staged interface of TrackingBatch, on the oracle-backed checker build
//     and on the product's host layer — the CPU-side twin that pins the core against the track table (host/track_table.cc), which is
//     itself pinned bit for bit against the reference's own tracking.cc (tests/golden/tracking_ref_*.npz).
// The state is the track table's, member for member (track_table.h): 72-byte feature rows in insertion order with the reference
// container's iteration order (HashOrder: libstdc++'s unordered_map node list and rehash policy), 64-byte map-point records with
// generation handles, observations as (frame, row), the window as (key, frame) pairs, frames freed by mark-and-sweep over the roots the
// reference's shared_ptrs form.  Capacities are compile-time (a stream is one flat block: upload / download / snapshot are memcpy);
// exceeding one sets Stream::overflow and the executor fails loudly.
//
// Every function cites the reference lines it follows; the floating-point expressions are written out operation by operation (both
// compilers run with -ffp-contract=off), so the two builds and the track table produce the same bits.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TC_FN __host__ __device__ inline
#else
#include <math.h>
#define TC_FN inline
#endif

namespace tc {

typedef unsigned long long u64;

// ---- execution model --------------------------------------------------------------------------------------------------------------------
// On the device a stage body is executed by ALL 64 lanes of the stream's wave.  Sequential bookkeeping is simply executed redundantly: the
// lanes run in lockstep, read the same addresses, compute the same values and store the same values — no guard is needed and none is
// written.  Data-parallel loops split their iterations over the lanes with the primitives below (chunks of NL items in order, ballot +
// rank for order-preserving appends), followed by sync() before any lane reads what another lane wrote.  The host build is the same source
// with NL == 1 (lane 0, ballot = the predicate, rank 0): every parallel loop degenerates to the plain sequential loop.
#if defined(__HIP_DEVICE_COMPILE__)
constexpr int NL = 64;
TC_FN int lane() { return (int) (threadIdx.x & 63); }
TC_FN u64 ballot(bool p) { return __ballot(p); }
TC_FN int popc(u64 m) { return __popcll(m); }
TC_FN u64 lanes_below() { return (1ull << lane()) - 1ull; }
TC_FN void sync() { // stores of every lane visible to every lane of the wave (same CU: ordering only, no cache maintenance)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
TC_FN u64 wave_sum(u64 v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// (round 5) scratch-memory atomics and an inclusive prefix sum over the lanes, for the parallel container-order construction
TC_FN uint32_t lds_min(uint32_t *p, uint32_t v) { return atomicMin(p, v); }
TC_FN uint32_t lds_add(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
TC_FN int32_t lds_exch(int32_t *p, int32_t v) { return atomicExch(p, v); }
TC_FN uint32_t wave_scan_incl(uint32_t v) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(v, o, 64);
        if (lane() >= o) v += up;
    }
    return v;
}
// the value another lane holds; `src` is the same in every lane (v_readlane: no LDS round trip)
TC_FN int lane_get(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
TC_FN double lane_get(double v, int src) {
    const u64 b = (u64) __double_as_longlong(v);
    const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) b, src), hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (b >> 32), src);
    return __longlong_as_double((long long) (((u64) hi << 32) | lo));
}
TC_FN int first_lane(u64 m) { return __ffsll((unsigned long long) m) - 1; }
TC_FN u64 wave_min(u64 v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 o = (u64) __shfl_xor((long long) v, m, 64);
        v           = o < v ? o : v;
    }
    return v;
}
TC_FN u64 wave_max(u64 v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const u64 o = (u64) __shfl_xor((long long) v, m, 64);
        v           = o > v ? o : v;
    }
    return v;
}
TC_FN uint32_t wave_or(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) v |= (uint32_t) __shfl_xor((int) v, m, 64);
    return v;
}
#if defined(TC_TIMING)
// profiling build only (csrc/Makefile EXTRA_HIPFLAGS=-DTC_TIMING, profiles/run_r05_call12.sh): wall-clock (100 MHz) time between marks,
// summed over the streams by lane 0 — where a stage's latency chain spends its time.  The product build compiles the marks away.
extern __device__ unsigned long long g_tc_marks[256];
__shared__ unsigned long long tc_last_mark;
TC_FN void tc_mark_start() {
    if (lane() == 0) tc_last_mark = wall_clock64();
}
TC_FN void tc_mark(int id) {
    const unsigned long long t = wall_clock64();
    if (lane() == 0) {
        atomicAdd(&g_tc_marks[id], t - tc_last_mark);
        atomicAdd(&g_tc_marks[128 + id], 1ull);
        tc_last_mark = t;
    }
}
#define TC_MARK(id) tc::tc_mark(id)
#define TC_MARK_START() tc::tc_mark_start()
#endif
#else
constexpr int NL = 1;
TC_FN int lane() { return 0; }
TC_FN u64 ballot(bool p) { return p ? 1ull : 0ull; }
TC_FN int popc(u64 m) { return (int) __builtin_popcountll(m); }
TC_FN u64 lanes_below() { return 0ull; }
TC_FN void sync() {}
TC_FN u64 wave_sum(u64 v) { return v; }
TC_FN uint32_t lds_min(uint32_t *p, uint32_t v) {
    const uint32_t o = *p;
    if (v < o) *p = v;
    return o;
}
TC_FN uint32_t lds_add(uint32_t *p, uint32_t v) {
    const uint32_t o = *p;
    *p               = o + v;
    return o;
}
TC_FN int32_t lds_exch(int32_t *p, int32_t v) {
    const int32_t o = *p;
    *p              = v;
    return o;
}
TC_FN uint32_t wave_scan_incl(uint32_t v) { return v; }
TC_FN int lane_get(int v, int) { return v; }
TC_FN double lane_get(double v, int) { return v; }
TC_FN int first_lane(u64 m) { return __builtin_ctzll(m); }
TC_FN u64 wave_min(u64 v) { return v; }
TC_FN u64 wave_max(u64 v) { return v; }
TC_FN uint32_t wave_or(uint32_t v) { return v; }
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define TC_UNROLL _Pragma("unroll")
#else
#define TC_UNROLL
#endif
#ifndef TC_MARK
#define TC_MARK(id) ((void) 0)
#define TC_MARK_START() ((void) 0)
#endif

// ---- capacities ------------------------------------------------------------------------------------------------------------------
constexpr int MAX_ROWS    = 640;   // features of one frame (C4: 500 + the detector's rounding slack), candidates, points of one LK call
constexpr int MAX_BUCKETS = 1109;  // libstdc++ bucket count after MAX_ROWS insertions (13, 29, 59, 127, 257, 541, 1109)
constexpr int MAX_FRAMES  = 28;    // live frames: window (<= 16 keyframes + 1) + cur / pre / ref / pending + candidates' reference frames
constexpr int MAX_MPS     = 8192;  // map-point pool (live landmarks of the window + the not yet inserted ones)
constexpr int MAX_WINDOW  = 18;    // keyframes in the map (window size + 1, rounded up)
constexpr int MAX_BLOCKS  = 64;    // detection grid blocks (C4: 50)
constexpr int MAX_TCW     = 12;    // distinct camera matrices of one triangulation call (current + reference frames of the candidates)
constexpr int LOG_CAP     = 8192;  // landmark insert / erase log between two host drains
constexpr int MAX_SLOTS   = 4;     // frame slots a stream owns on the device (pre / cur / ref / incoming)

// per-wave scratch (LDS on the device, a heap block on the host): the linked lists and hash buckets of the frame a stage is working on,
// so that the sequential walks / insertions chase pointers through LDS instead of HBM
struct Scratch {
    int32_t next[MAX_ROWS];
    int32_t bucket[MAX_BUCKETS];
    int32_t tmp_bucket[MAX_BUCKETS];
    u64 key[MAX_ROWS];
    uint32_t want[MAX_ROWS + 2]; // bucket counts after k insertions for the rows an order_extend pass enters (a copy of buckets_after)
    uint16_t ibkt[MAX_ROWS];     // order_extend: the bucket of row i under the bucket count in effect at ITS insertion (computed in parallel)
    uint16_t rbkt[MAX_ROWS];     // order_extend: the bucket of node p under the bucket count a rehash moves to (computed in parallel)
    // order_extend_parallel (round 5): per bucket the head of an (unordered) event list; per event its link, per time the chain sizes /
    // their suffix sums; the list order as an array, twice (a phase reads one and writes the other)
    int32_t bhead[MAX_BUCKETS];
    int32_t lnk[MAX_ROWS];
    uint32_t tsum[MAX_ROWS + 1];
    uint16_t ord[2][MAX_ROWS];
};

enum { TRACK_FIRST_FRAME = 0, TRACK_INITIALIZING = 1, TRACK_TRACKING = 2, TRACK_PASSED = 3, TRACK_LOST = 4 }; // tracking.h:38-44
enum { KEYFRAME_NONE = 0, KEYFRAME_REMOVE_SECOND_NEW = 1, KEYFRAME_NORMAL = 2, KEYFRAME_REMOVE_OLDEST = 3 }; // frame.h:36-41
enum { FEATURE_MATCHED = 0, FEATURE_TRIANGULATED = 1 };
enum { MAPPOINT_TRIANGULATED = 0 }; // mappoint.h:36-42
enum { M_NONE = 0, M_FIRST = 1, M_INIT = 2, M_TRACK = 3 };
enum { OVF_ROWS = 1, OVF_FRAMES = 2, OVF_MPS = 4, OVF_TCW = 8, OVF_LOG = 16, OVF_WINDOW = 32, OVF_SLOTS = 64, OVF_INTERNAL = 128 };

// ---- records (layouts shared with track_table.h: static_asserts there and here) -----------------------------------------------------
struct P2f {
    float x, y;
};
struct Row { // one Feature (feature.h:41-118)
    u64 id;
    uint32_t mp, mpgen;
    P2f kp, kpd;
    double vel[2];
    double pcx, pcy;
    int32_t lk_idx;
    int8_t type;
    uint8_t outlier;
    uint8_t pad_[2];
};
static_assert(sizeof(Row) == 72, "feature row");
struct LastObs {
    int32_t frame;
    uint32_t gen;
    int32_t row;
};
struct alignas(64) MpHot {
    uint32_t gen;
    uint8_t live, outlier, in_map;
    int8_t type;
    u64 id;
    double pos[3];
    int32_t observed, used;
    LastObs last;
};
static_assert(sizeof(MpHot) == 64, "hot map-point record");
struct MpCold {
    u64 born_fid;
    int32_t ref_frame;
    uint32_t ref_gen;
    P2f ref_kp;
    double depth;
    int32_t optimized;
    int32_t pad_;
};
static_assert(sizeof(MpCold) == 40, "cold map-point record");
struct MpRef {
    uint32_t i, g;
};
struct Pose {
    double R[9]; // row-major
    double t[3];
};

struct Frame {
    int32_t alive;
    uint32_t gen;
    u64 fid, kf_id;
    double stamp;
    Pose pose;
    int32_t is_kf, kf_state, slot;
    u64 image; // address of the frame's raw image as the caller handed it in (host or device memory); only the B2 view needs it
    // rows in insertion order + the container order of the reference's features_ (HashOrder)
    int32_t n_rows, head, n_buckets, n_unupd;
    u64 magic;
    Row row[MAX_ROWS];
    int32_t next[MAX_ROWS];
    int32_t bucket[MAX_BUCKETS];
    uint32_t unupd[MAX_ROWS], unupd_gen[MAX_ROWS]; // frame.h unupdated_mappoints_
};

struct LmLog { // Map::landmarks_ operation history since the last drain: the host replays it into its container (track_table.h map_lm_)
    u64 id;
    uint32_t mp;
    int32_t op; // 1 insert, 0 erase
};

// ---- configuration (constant per batch) ----------------------------------------------------------------------------------------------
struct Cam {
    double fx, fy, cx, cy, skew, k1, k2, p1, p2, k3;
    int32_t width, height;
};
struct Cfg {
    Cam cam;
    int32_t track_max_features, check_histogram, window_size, pad0_;
    double track_min_parallax, reprojection_error_std, track_max_interval /* x 0.95 (tracking.cc:57) */;
    int32_t block_cols, block_rows, block_cnts, block_w, block_h, max_block_features, min_pixel_distance, max_per_job;
    u64 stream_id_base; // unused by the algorithm (per-stream id spaces start at 0); kept for the executor
};

// ---- per-stream I/O with the device primitives (the executor points these at the stream's segment of the group arenas) -----------------
struct Io {
    // F1 preprocess
    int32_t *pre_slot;     // [1] slot the incoming frame is preprocessed into (-1: no frame this step)
    const double *pre_hist; // [1] mean brightness of the raw frame (histogram gate), valid when Cfg::check_histogram
    // F2/F3/F4 LK forward-backward + undistortion
    int32_t *lk_count;      // [1]
    int32_t *lk_prev_slot, *lk_next_slot; // [MAX_ROWS]
    P2f *lk_prev, *lk_guess;              // [MAX_ROWS]
    const P2f *lk_out, *lk_undist;        // [MAX_ROWS]
    const uint8_t *lk_status;             // [MAX_ROWS]
    int32_t lk_base;                      // index of this stream's first point in the group's LK call (set-up reuse hints)
    // F6 RANSAC (one set per stream)
    int32_t *rs_count; // [1] 0: no set
    P2f *rs_p1, *rs_p2;
    const uint8_t *rs_mask;
    // F8 triangulation
    int32_t *tri_count, *tri_n_tcw;
    int32_t *tri_T0, *tri_T1; // [MAX_ROWS] indices into this stream's tri_Tcw table
    double *tri_Tcw;          // [MAX_TCW][12]
    double *tri_pc0, *tri_pc1; // [MAX_ROWS][3]
    const double *tri_pw;      // [MAX_ROWS][3]
    // F7 detection (one job per stream)
    int32_t *det_slot;     // [1] -1: no job
    int32_t *det_quota;    // [block_cnts]
    int32_t *det_mask_count;
    P2f *det_mask_pts;     // [MAX_ROWS]
    const int32_t *det_count;
    const P2f *det_out;    // [max_per_job]
};

// ---- the stream --------------------------------------------------------------------------------------------------------------------
struct Stream {
    // id factories (frame.cc:37-53, mappoint.cc:45-49): one id space per stream
    u64 frame_id, keyframe_id, mappoint_id;
    // tracker roles (handles into frame[]; -1 = none)
    int32_t cur, ref, pre, last_keyframe, pending, latest_keyframe, det_frame;
    int32_t overflow;
    // frame pool
    int32_t n_frames, n_free_frames;
    int32_t free_frames[MAX_FRAMES];
    // map (tracking/map.cc)
    int32_t n_map_kf, is_window_full, n_landmarks, pad1_;
    u64 map_kf_key[MAX_WINDOW];
    int32_t map_kf_frame[MAX_WINDOW];
    // tracker scalars (tracking.h:117-160)
    double parallax_map, parallax_ref, histogram;
    int32_t parallax_map_counts, parallax_ref_counts, isnewkeyframe, isinitializing, passed_cnt;
    // per-frame staged state
    int32_t done, result, pending_slot, mode, det_job, det_ismask, lk_map_begin, lk_map_n, lk_ref_begin, lk_ref_n, ref_tracked, rs_set, kf_state,
        tri_queued, lost_reset, tri_begin;
    u64 last_input_fid;
    // the tracking.txt line of a keyframe decision (tracking.cc:289-296, 309-315): stamp, dt, parallax, relative translation, relative
    // rotation [deg]; written out by the host executor when a log file is configured (log_valid: set at the decision, cleared per frame)
    double log_data[5];
    int32_t log_valid, pad3_;
    int32_t n_owned, owned_slots[MAX_SLOTS + 1], n_free_slots, free_slots[MAX_SLOTS];
    // candidate lists (tracking.h:129-136) and their carried twins; every list keeps its own length, as the vectors of the table do
    int32_t n_cur, n_new, n_ref, n_ref_undis, n_new_undis, n_ref_frame, n_cand_lk, n_vel_ref, n_vel_cur, n_tracked, n_matched, n_tr_new_undis,
        n_tr_cur_undis, n_tri_status, n_tri_index, n_tri_ref_undis, n_tri_cur_undis;
    P2f pts2d_cur[MAX_ROWS], pts2d_new[MAX_ROWS], pts2d_ref[MAX_ROWS], pts2d_ref_undis[MAX_ROWS], pts2d_new_undis[MAX_ROWS];
    int32_t pts2d_ref_frame[MAX_ROWS], cand_lk_idx[MAX_ROWS];
    double velocity_ref[MAX_ROWS][2], velocity_cur[MAX_ROWS][2];
    MpRef tracked_mappoint[MAX_ROWS], mappoint_matched[MAX_ROWS];
    double tm_pc[MAX_ROWS][2];
    P2f tr_new_undis[MAX_ROWS], tr_cur_undis[MAX_ROWS], tri_ref_undis[MAX_ROWS], tri_cur_undis[MAX_ROWS], scratch_a[MAX_ROWS];
    int32_t tri_point_index[MAX_ROWS];
    uint8_t tri_status[MAX_ROWS], status[MAX_ROWS];
    int32_t order_idx[MAX_ROWS];
    int32_t scratch_bucket[MAX_BUCKETS];
    double tri_tmp[MAX_ROWS][4]; // normalized points of the candidates a triangulation takes (reference view x, y; current view x, y)
    double par_term[MAX_ROWS]; // terms of a parallax average in the order they are summed (computed in parallel, summed sequentially)
    uint8_t par_ok[MAX_ROWS];
    // statistics / digest (TrackingBatch::Stream)
    u64 frames, keyframes, tracked_sum, digest;
    int32_t last_state, pad2_;
    // landmark container history
    int32_t n_log, log_dropped;
    LmLog log[LOG_CAP];
    // pools
    int32_t n_mps, n_free_mps;
    uint32_t free_mps[MAX_MPS];
    MpHot hot[MAX_MPS];
    MpCold cold[MAX_MPS];
    Frame frame[MAX_FRAMES];
};

// ---- small math, written out (types.h / model.h twins) ---------------------------------------------------------------------------------
TC_FN double tc_sqrt(double v) { return sqrt(v); }
TC_FN double tc_fabs(double v) { return fabs(v); }

TC_FN void mat_mul_t(const double *A, const double *B, double *out) { // A^T * B (Matrix3d::transpose() then operator*)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) out[i * 3 + j] = A[0 * 3 + i] * B[0 * 3 + j] + A[1 * 3 + i] * B[1 * 3 + j] + A[2 * 3 + i] * B[2 * 3 + j];
}
TC_FN void world2cam(const double *pw, const Pose &pose, double *pc) { // camera.cc:145-147: pose.R^T * (world - pose.t)
    const double d0 = pw[0] - pose.t[0], d1 = pw[1] - pose.t[1], d2 = pw[2] - pose.t[2];
    const double *R = pose.R;
    pc[0] = R[0] * d0 + R[3] * d1 + R[6] * d2;
    pc[1] = R[1] * d0 + R[4] * d1 + R[7] * d2;
    pc[2] = R[2] * d0 + R[5] * d1 + R[8] * d2;
}
TC_FN void pixel2cam(const Cam &c, const P2f &p, double &x, double &y) { // camera.cc:123-127
    y = (p.y - c.cy) / c.fy;
    x = (p.x - c.cx - c.skew * y) / c.fx;
}
TC_FN P2f cam2pixel(const Cam &c, double X, double Y, double Z) { // camera.cc:129-131
    P2f r;
    r.x = (float) ((c.fx * X + c.skew * Y) / Z + c.cx);
    r.y = (float) (c.fy * Y / Z + c.cy);
    return r;
}
TC_FN P2f world2pixel(const Cam &c, const double *pw, const Pose &pose) {
    double pc[3];
    world2cam(pw, pose, pc);
    return cam2pixel(c, pc[0], pc[1], pc[2]);
}
TC_FN void distortPoint(const Cam &c, P2f &pp) { // camera.cc:91-102
    double x, y;
    pixel2cam(c, pp, x, y);
    const double r2 = x * x + y * y;
    const double rr = (1 + c.k1 * r2 + c.k2 * r2 * r2 + c.k3 * r2 * r2 * r2);
    const double xd = x * rr + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
    const double yd = y * rr + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
    pp              = cam2pixel(c, xd, yd, 1.0);
}
TC_FN P2f distortCameraPoint(const Cam &c, double X, double Y, double Z) { // camera.cc:104-117
    const double x = X / Z, y = Y / Z;
    const double r2 = x * x + y * y;
    const double rr = (1 + c.k1 * r2 + c.k2 * r2 * r2 + c.k3 * r2 * r2 * r2);
    const double a  = (double) (float) (x * rr + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x));
    const double b  = (double) (float) (y * rr + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y);
    return cam2pixel(c, a, b, 1.0);
}
// cv::undistortPoints(pts, pts, K, D, noArray, K) for one point (model.cc Camera::undistortPoints, csrc/dev_camera.h)
TC_FN P2f undistortPoint(const Cam &c, const P2f &p) {
    const double ifx = 1. / c.fx, ify = 1. / c.fy;
    double x = p.x, y = p.y;
    const double u = x, v = y;
    x               = (x - c.cx) * ifx;
    y               = (y - c.cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2     = x * x + y * y;
        const double icdist = 1. / (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        if (icdist < 0) {
            x = (u - c.cx) * ifx;
            y = (v - c.cy) * ify;
            break;
        }
        const double deltaX = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
        const double deltaY = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
        x                   = (x0 - deltaX) * icdist;
        y                   = (y0 - deltaY) * icdist;
    }
    P2f r;
    r.x = (float) (c.fx * x + c.skew * y + c.cx);
    r.y = (float) (c.fy * y + c.cy);
    return r;
}
TC_FN double focalLength(const Cam &c) { return (c.fx + c.fy) * 0.5; }

// ---- HashOrder (track_table.cc: bits/hashtable.h _M_insert_unique_node / _M_insert_bucket_begin / _M_rehash_aux) ---------------------
constexpr int H_EMPTY = -1, H_BEFORE_BEGIN = -2;

TC_FN u64 mulhi64(u64 a, u64 b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (u64) (((unsigned __int128) a * b) >> 64);
#endif
}
TC_FN u64 modMagic(u64 n) { return 0xFFFFFFFFFFFFFFFFull / n + 1; }
TC_FN int bucketOf(u64 key, int n, u64 M) {
    if ((key >> 32) != 0) return (int) (key % (u64) n);
    const u64 low = M * (u64) (uint32_t) key;
    return (int) mulhi64(low, (u64) n);
}
TC_FN void order_clear(Frame &f) {
    f.n_rows    = 0;
    f.head      = -1;
    f.n_buckets = 1;
    f.bucket[0] = H_EMPTY;
    f.magic     = 0; // (M for one bucket is 2^64: wraps to 0, and the fastmod of any key is 0 — the right bucket)
}
TC_FN int order_next_of(const Frame &f, int prev) { return prev == H_BEFORE_BEGIN ? f.head : f.next[prev]; }
TC_FN void order_set_next(Frame &f, int prev, int i) {
    if (prev == H_BEFORE_BEGIN)
        f.head = i;
    else
        f.next[prev] = i;
}
TC_FN bool order_contains(const Frame &f, u64 key) {
    const int n = f.n_buckets, b = bucketOf(key, n, f.magic);
    const int prev = f.bucket[b];
    if (prev == H_EMPTY) return false;
    for (int p = order_next_of(f, prev); p >= 0 && bucketOf(f.row[p].id, n, f.magic) == b; p = f.next[p])
        if (f.row[p].id == key) return true;
    return false;
}
TC_FN void order_rehash(Frame &f, int n, int32_t *scratch) {
    for (int b = 0; b < n; b++) scratch[b] = H_EMPTY;
    const u64 M = modMagic((u64) n);
    int p = f.head;
    f.head = -1;
    int bbegin_bkt = 0;
    while (p >= 0) {
        const int nx = f.next[p];
        const int b  = bucketOf(f.row[p].id, n, M);
        if (scratch[b] == H_EMPTY) {
            f.next[p]  = f.head;
            f.head     = p;
            scratch[b] = H_BEFORE_BEGIN;
            if (f.next[p] >= 0) scratch[bbegin_bkt] = p;
            bbegin_bkt = b;
        } else {
            const int prev = scratch[b];
            f.next[p]      = order_next_of(f, prev);
            order_set_next(f, prev, p);
        }
        p = nx;
    }
    for (int b = 0; b < n; b++) f.bucket[b] = scratch[b];
    f.n_buckets = n;
    f.magic     = modMagic((u64) n);
}
// row index n_rows (the caller has filled f.row[n_rows].id) enters the container order; buckets_after[k] = bucket count of a fresh
// std::unordered_map<ulong, char> after k insertions (HashOrder::bucketsAfter)
TC_FN void order_insert_unique(Frame &f, const uint32_t *buckets_after, int32_t *scratch) {
    const int i    = f.n_rows;
    const int want = (int) buckets_after[i + 1];
    if (want != f.n_buckets) order_rehash(f, want, scratch);
    const int n = f.n_buckets, b = bucketOf(f.row[i].id, n, f.magic);
    f.next[i]   = -1;
    if (f.bucket[b] != H_EMPTY) {
        const int prev = f.bucket[b];
        f.next[i]      = order_next_of(f, prev);
        order_set_next(f, prev, i);
    } else {
        f.next[i] = f.head;
        f.head    = i;
        if (f.next[i] >= 0) f.bucket[bucketOf(f.row[f.next[i]].id, n, f.magic)] = i;
        f.bucket[b] = H_BEFORE_BEGIN;
    }
    f.n_rows = i + 1;
}

// ---- pools (track_table.cc) ----------------------------------------------------------------------------------------------------------
TC_FN bool mp_valid(const Stream &S, uint32_t i, uint32_t g) { return S.hot[i].live && S.hot[i].gen == g; }
TC_FN void mp_release(Stream &S, uint32_t i) {
    S.hot[i].live = 0;
    S.hot[i].gen++;
    S.free_mps[S.n_free_mps++] = i;
}
TC_FN uint32_t mp_alloc(Stream &S) {
    uint32_t i;
    if (S.n_free_mps > 0) {
        i = S.free_mps[--S.n_free_mps];
    } else if (S.n_mps < MAX_MPS) {
        i = (uint32_t) S.n_mps++;
        S.hot[i].gen = 0;
    } else {
        S.overflow |= OVF_MPS;
        i = MAX_MPS - 1; // (in bounds; the executor fails the step)
    }
    const uint32_t g = S.hot[i].gen;
    MpHot h;
    memset(&h, 0, sizeof h);
    h.gen  = g;
    h.live = 1;
    h.last.frame = -1;
    h.last.row   = -1;
    S.hot[i] = h;
    MpCold c;
    memset(&c, 0, sizeof c);
    c.ref_frame = -1;
    S.cold[i]   = c;
    return i;
}
TC_FN void frame_clear_rows(Frame &f) {
    order_clear(f);
    f.n_unupd = 0;
}
TC_FN int frame_alloc(Stream &S) {
    int h;
    if (S.n_free_frames > 0) {
        h = S.free_frames[--S.n_free_frames];
    } else if (S.n_frames < MAX_FRAMES) {
        h = S.n_frames++;
        S.frame[h].gen = 0;
    } else {
        S.overflow |= OVF_FRAMES;
        h = MAX_FRAMES - 1;
    }
    Frame &f   = S.frame[h];
    f.alive    = 1;
    f.fid      = 0;
    f.kf_id    = 0;
    f.is_kf    = 0;
    f.kf_state = KEYFRAME_NORMAL;
    f.slot     = -1;
    f.image    = 0;
    frame_clear_rows(f);
    return h;
}
// mp_release for the map points of a frame's unupdated list that the map does not hold (Frame::clearFeatures, frame.h:46-51), in list order:
// a chunk of entries per step; what the one-by-one loop pushes onto the free list in sequence is a function of the entry's rank among the
// released ones (the entries of one list are distinct map points)
TC_FN void release_unupdated(Stream &S, const Frame &f) {
    const int free0 = S.n_free_mps;
    int n_rel       = 0;
    for (int base = 0; base < f.n_unupd; base += NL) {
        const int k = base + lane();
        bool rel    = false;
        uint32_t i  = 0;
        if (k < f.n_unupd) {
            i   = f.unupd[k];
            rel = mp_valid(S, i, f.unupd_gen[k]) && !S.hot[i].in_map;
        }
        const u64 m = ballot(rel);
        if (rel) {
            S.hot[i].live = 0;
            S.hot[i].gen++;
            S.free_mps[free0 + n_rel + popc(m & lanes_below())] = i;
        }
        n_rel += popc(m);
    }
    S.n_free_mps = free0 + n_rel;
    sync();
}
TC_FN void frame_free(Stream &S, int h) {
    Frame &f = S.frame[h];
    // a map point lives as long as the map or a frame's unupdated list holds it; this frame's list goes away with it
    release_unupdated(S, f);
    f.alive = 0;
    f.gen++;
    f.image = 0;
    frame_clear_rows(f);
    S.free_frames[S.n_free_frames++] = h;
}
// A Frame of the reference dies with its last shared_ptr: the tracker's roles, the candidates' reference frames, the map.
TC_FN void sweep_frames(Stream &S) {
    uint32_t mark = 0; // MAX_FRAMES <= 32
    if (S.cur >= 0) mark |= 1u << S.cur;
    if (S.pre >= 0) mark |= 1u << S.pre;
    if (S.ref >= 0) mark |= 1u << S.ref;
    if (S.last_keyframe >= 0) mark |= 1u << S.last_keyframe;
    if (S.pending >= 0) mark |= 1u << S.pending;
    if (S.latest_keyframe >= 0) mark |= 1u << S.latest_keyframe;
    if (S.det_frame >= 0) mark |= 1u << S.det_frame;
    // the map's keyframes, the candidates' reference frames (a chunk of entries per step), then the live frames nobody marked
    for (int base = 0; base < S.n_map_kf; base += NL) {
        const int k = base + lane();
        mark |= wave_or(k < S.n_map_kf ? 1u << S.map_kf_frame[k] : 0u);
    }
    for (int base = 0; base < S.n_ref_frame; base += NL) {
        const int k = base + lane();
        mark |= wave_or(k < S.n_ref_frame ? 1u << S.pts2d_ref_frame[k] : 0u);
    }
    uint32_t dead = 0;
    for (int base = 0; base < S.n_frames; base += NL) {
        const int h = base + lane();
        dead |= wave_or((h < S.n_frames && S.frame[h].alive && !((mark >> h) & 1u)) ? 1u << h : 0u);
    }
    for (int h = 0; h < S.n_frames; h++) // (in handle order, as the one-by-one scan frees them)
        if ((dead >> h) & 1u) frame_free(S, h);
}
static_assert(MAX_FRAMES <= 32, "sweep_frames marks frames in one 32-bit word");

TC_FN void set_keyframe(Stream &S, int h, int state) { // frame.cc:42-54
    Frame &f = S.frame[h];
    if (!f.is_kf) {
        f.is_kf    = 1;
        f.kf_id    = S.keyframe_id++;
        f.kf_state = state;
    }
}
// appends a row to frame h (the key is known to be absent: ids of the previous frame's rows, freshly drawn ids); returns its index
TC_FN int add_row(Stream &S, int h, u64 id, uint32_t mp, const P2f &kp, const P2f &kpd, double vx, double vy, int type, double pcx, double pcy,
                  int32_t lk_idx, const uint32_t *buckets_after) {
    Frame &f = S.frame[h];
    if (f.n_rows >= MAX_ROWS) {
        S.overflow |= OVF_ROWS;
        return MAX_ROWS - 1;
    }
    Row r;
    r.id      = id;
    r.mp      = mp;
    r.mpgen   = S.hot[mp].gen;
    r.kp      = kp;
    r.kpd     = kpd;
    r.vel[0]  = vx;
    r.vel[1]  = vy;
    r.pcx     = pcx;
    r.pcy     = pcy;
    r.lk_idx  = lk_idx;
    r.type    = (int8_t) type;
    r.outlier = 0;
    r.pad_[0] = r.pad_[1] = 0;
    const int i = f.n_rows;
    f.row[i]    = r;
    order_insert_unique(f, buckets_after, S.scratch_bucket);
    return i;
}
// the row data only (the caller enters the new rows into the container order afterwards: order_extend)
TC_FN int append_row(Stream &S, int h, u64 id, uint32_t mp, const P2f &kp, const P2f &kpd, double vx, double vy, int type, double pcx, double pcy,
                     int32_t lk_idx) {
    Frame &f = S.frame[h];
    if (f.n_rows >= MAX_ROWS) {
        S.overflow |= OVF_ROWS;
        return MAX_ROWS - 1;
    }
    Row r;
    r.id      = id;
    r.mp      = mp;
    r.mpgen   = S.hot[mp].gen;
    r.kp      = kp;
    r.kpd     = kpd;
    r.vel[0]  = vx;
    r.vel[1]  = vy;
    r.pcx     = pcx;
    r.pcy     = pcy;
    r.lk_idx  = lk_idx;
    r.type    = (int8_t) type;
    r.outlier = 0;
    r.pad_[0] = r.pad_[1] = 0;
    const int i = f.n_rows;
    f.row[i]    = r;
    f.n_rows    = i + 1;
    return i;
}
TC_FN void log_landmark(Stream &S, u64 id, uint32_t mp, int op) {
    if (S.n_log >= LOG_CAP) {
        S.overflow |= OVF_LOG;
        S.log_dropped++;
        return;
    }
    LmLog e;
    e.id = id, e.mp = mp, e.op = op;
    S.log[S.n_log++] = e;
}

// ---- map (tracking/map.cc) on handles -----------------------------------------------------------------------------------------------
TC_FN int map_find(const Stream &S, u64 key) {
    for (int k = 0; k < S.n_map_kf; k++)
        if (S.map_kf_key[k] == key) return k;
    return -1;
}
TC_FN bool map_is_keyframe_in_map(const Stream &S, int h) { return map_find(S, S.frame[h].kf_id) >= 0; }
// the same look-up by the whole wave (every lane calls it with the same key): an entry per lane, one memory round trip instead of one per entry
TC_FN int map_find_wave(const Stream &S, u64 key) {
    for (int base = 0; base < S.n_map_kf; base += NL) {
        const int k = base + lane();
        const u64 m = ballot(k < S.n_map_kf && S.map_kf_key[k] == key);
        if (m) return base + first_lane(m);
    }
    return -1;
}
TC_FN void map_insert_keyframe(Stream &S, const Cfg &C, int h) { // map.cc:27-61
    S.latest_keyframe = h;
    Frame &f          = S.frame[h];
    const int at      = map_find_wave(S, f.kf_id);
    if (at < 0) {
        if (S.n_map_kf >= MAX_WINDOW) {
            S.overflow |= OVF_WINDOW;
        } else {
            S.map_kf_key[S.n_map_kf]   = f.kf_id;
            S.map_kf_frame[S.n_map_kf] = h;
            S.n_map_kf++;
        }
    } else {
        S.map_kf_frame[at] = h;
    }
    // the frame's new map points enter the map (map.cc:56-61), in list order: a chunk per step, the history entries by rank
    int n_in = 0;
    const int log0 = S.n_log;
    for (int base = 0; base < f.n_unupd; base += NL) {
        const int k = base + lane();
        bool in     = false;
        uint32_t i  = 0;
        if (k < f.n_unupd) {
            i  = f.unupd[k];
            in = mp_valid(S, i, f.unupd_gen[k]) && !S.hot[i].in_map;
        }
        const u64 m = ballot(in);
        if (in) {
            S.hot[i].in_map = 1;
            const int at    = log0 + n_in + popc(m & lanes_below());
            if (at < LOG_CAP) {
                LmLog e;
                e.id = S.hot[i].id, e.mp = i, e.op = 1;
                S.log[at] = e;
            }
        }
        n_in += popc(m);
    }
    if (log0 + n_in > LOG_CAP) {
        S.overflow |= OVF_LOG;
        S.log_dropped += log0 + n_in - LOG_CAP;
        S.n_log = LOG_CAP;
    } else {
        S.n_log = log0 + n_in;
    }
    S.n_landmarks += n_in;
    sync();
    if (S.n_map_kf > C.window_size) S.is_window_full = 1;
}
TC_FN void map_remove_keyframe(Stream &S, int h, bool isremovemappoint) { // map.cc:89-127
    Frame &f = S.frame[h];
    if (isremovemappoint) {
        // the landmarks this keyframe is the reference frame of leave the map: found in parallel (a chunk of rows per step, appended in row
        // order), released one by one in that order
        int n_rm = 0;
        for (int base = 0; base < f.n_rows; base += NL) {
            const int q = base + lane();
            bool rm     = false;
            uint32_t i  = 0;
            if (q < f.n_rows) {
                const Row &r = f.row[q];
                i            = r.mp;
                rm           = mp_valid(S, i, r.mpgen) && S.cold[i].ref_frame == h && S.cold[i].ref_gen == f.gen && S.hot[i].in_map;
            }
            const u64 m = ballot(rm);
            if (rm) S.order_idx[n_rm + popc(m & lanes_below())] = (int32_t) i;
            n_rm += popc(m);
        }
        sync();
        // ... released in that order, a chunk per step: the history entry and the free-list slot of a landmark are its rank among the released
        // (the rows of one frame hold distinct map points)
        const int log0 = S.n_log, free0 = S.n_free_mps;
        int n_ok = 0;
        for (int base = 0; base < n_rm; base += NL) {
            const int q = base + lane();
            bool ok     = false;
            uint32_t i  = 0;
            if (q < n_rm) {
                i  = (uint32_t) S.order_idx[q];
                ok = S.hot[i].live && S.hot[i].in_map;
            }
            const u64 m = ballot(ok);
            if (ok) {
                const int r      = n_ok + popc(m & lanes_below());
                S.hot[i].in_map  = 0;
                S.hot[i].outlier = 1;
                if (log0 + r < LOG_CAP) { // log_landmark(S, id, i, 0)
                    LmLog e;
                    e.id = S.hot[i].id, e.mp = i, e.op = 0;
                    S.log[log0 + r] = e;
                }
                S.hot[i].live = 0; // mp_release(S, i)
                S.hot[i].gen++;
                S.free_mps[free0 + r] = i;
            }
            n_ok += popc(m);
        }
        if (log0 + n_ok > LOG_CAP) {
            S.overflow |= OVF_LOG;
            S.log_dropped += log0 + n_ok - LOG_CAP;
            S.n_log = LOG_CAP;
        } else {
            S.n_log = log0 + n_ok;
        }
        S.n_landmarks -= n_ok;
        S.n_free_mps = free0 + n_ok;
        sync();
        release_unupdated(S, f); // Frame::clearFeatures (frame.h:46-51)
        frame_clear_rows(f);
    }
    const int at = map_find_wave(S, f.kf_id);
    if (at >= 0) { // vector::erase: the later entries move down (a chunk of entries per step: loaded, then stored one place lower)
        const int n = S.n_map_kf;
        for (int base = at; base + 1 < n; base += NL) {
            const int k    = base + lane();
            const bool mv  = k + 1 < n;
            const u64 key  = mv ? S.map_kf_key[k + 1] : 0;
            const int fr   = mv ? S.map_kf_frame[k + 1] : 0;
            sync(); // (every lane has read its successor before any lane overwrites it)
            if (mv) S.map_kf_key[k] = key, S.map_kf_frame[k] = fr;
            sync();
        }
        S.n_map_kf = n - 1;
    }
}

// ---- device slots (per-stream pool of MAX_SLOTS) --------------------------------------------------------------------------------------
TC_FN int slot_alloc(Stream &S) {
    if (S.n_free_slots <= 0) {
        S.overflow |= OVF_SLOTS;
        return S.free_slots[0];
    }
    return S.free_slots[--S.n_free_slots];
}
TC_FN void slot_free(Stream &S, int s) { S.free_slots[S.n_free_slots++] = s; }
TC_FN void assign_slot(Stream &S, int h) {
    S.frame[h].slot               = S.pending_slot;
    S.owned_slots[S.n_owned++]    = S.pending_slot;
    S.pending_slot                = -1;
}
TC_FN void release_unused_slots(Stream &S) {
    // (the roles' slots are read once: the loop's stores cannot change them, but the compiler must assume they do and would re-read the
    // handles and the frames — six dependent loads — for every owned slot)
    const int cur = S.cur, pre = S.pre, ref = S.ref, n_owned = S.n_owned;
    const int s_cur = cur >= 0 ? S.frame[cur].slot : -1, s_pre = pre >= 0 ? S.frame[pre].slot : -1, s_ref = ref >= 0 ? S.frame[ref].slot : -1;
    int owned[MAX_SLOTS + 1];
    for (int k = 0; k < MAX_SLOTS + 1; k++) owned[k] = k < n_owned ? S.owned_slots[k] : -1;
    int keep = 0, n_free = S.n_free_slots;
    for (int k = 0; k < MAX_SLOTS + 1; k++) {
        if (k >= n_owned) break;
        const int s     = owned[k];
        const bool used = (cur >= 0 && s_cur == s) || (pre >= 0 && s_pre == s) || (ref >= 0 && s_ref == s);
        if (used)
            S.owned_slots[keep++] = s;
        else
            S.free_slots[n_free++] = s; // slot_free(S, s)
    }
    S.n_free_slots = n_free;
    S.n_owned      = keep;
}

// ---- helpers (tracking.cc:813-871) ------------------------------------------------------------------------------------------------------
// reduceVector (:831-839): stable in-place compaction; chunks of NL items in order — a chunk's writes land at or below its own first index,
// later chunks read above it, and inside a chunk every store waits for the loads (its data comes from one)
template <typename T> TC_FN int reduce_vector(T *vec, int n, const uint8_t *status) {
    int index = 0;
    for (int base = 0; base < n; base += NL) {
        const int k     = base + lane();
        const bool keep = k < n && status[k];
        T v             = vec[keep ? k : 0];
        const u64 m     = ballot(keep);
        if (keep) vec[index + popc(m & lanes_below())] = v;
        index += popc(m);
    }
    sync();
    return index;
}
struct D2 {
    double a, b;
};
TC_FN int reduce_vector2(double (*vec)[2], int n, const uint8_t *status) { return reduce_vector(reinterpret_cast<D2 *>(vec), n, status); }
// Several lists compacted by ONE status vector (the reference calls reduceVector on each in turn, :507-511 / :550-554 / :788-793): a chunk's
// status is read once, every list's element of the chunk is loaded before any is stored — one memory round trip per chunk instead of one per
// chunk and list, one sync() instead of one per list.  Each list keeps its own length (k < n of that list, as its own call would).
template <typename T> struct Compact {
    T *vec;
    int n, kept;
    bool mine;
    T v;
    TC_FN void load(int k, bool keep) {
        mine = keep && k < n;
        v    = vec[mine ? k : 0];
    }
    TC_FN void store(int pos) {
        if (mine) vec[pos] = v;
        kept += popc(ballot(mine));
    }
};
template <typename T> TC_FN Compact<T> compact(T *vec, int n) {
    Compact<T> c;
    c.vec = vec, c.n = n, c.kept = 0, c.mine = false;
    return c;
}
TC_FN Compact<D2> compact2(double (*vec)[2], int n) { return compact(reinterpret_cast<D2 *>(vec), n); }
template <typename... C> TC_FN void reduce_vectors(const uint8_t *status, C &...c) {
    int nmax = 0;
    ((nmax = c.n > nmax ? c.n : nmax), ...);
    int index = 0;
    for (int base = 0; base < nmax; base += NL) {
        const int k     = base + lane();
        const bool keep = k < nmax && status[k];
        const u64 m     = ballot(keep);
        const int pos   = index + popc(m & lanes_below());
        (c.load(k, keep), ...);
        (c.store(pos), ...);
        index += popc(m);
    }
    sync();
}
template <typename T> TC_FN void copy_n(T *dst, const T *src, int n) {
    for (int k = lane(); k < n; k += NL) dst[k] = src[k];
    sync();
}
TC_FN bool is_good_to_track(const Cfg &C, const P2f &pp, const Pose &pose, const double *pw, double scale, double depth_scale) { // :813-829
    double pc[3];
    world2cam(pw, pose, pc);
    if (!((pc[2] > 1.0 /*NEAREST_DEPTH*/) && (pc[2] < 200.0 /*FARTHEST_DEPTH*/ * depth_scale))) return false; // :247-249
    const P2f ppp   = cam2pixel(C.cam, pc[0], pc[1], pc[2]);
    const double ex = ppp.x - pp.x, ey = ppp.y - pp.y; // Vector2d of float differences (camera.cc:153-157)
    if (tc_sqrt(ex * ex + ey * ey) > C.reprojection_error_std * scale) return false;
    return true;
}
TC_FN double keypoint_parallax(const Cfg &C, const P2f &pp0, const P2f &pp1, const double *R10) { // :861-871
    double x0, y0, x1, y1;
    pixel2cam(C.cam, pp0, x0, y0);
    pixel2cam(C.cam, pp1, x1, y1);
    const double a = R10[0] * x0 + R10[1] * y0 + R10[2] * 1.0, b = R10[3] * x0 + R10[4] * y0 + R10[5] * 1.0;
    const double dx = a - x1, dy = b - y1;
    return tc_sqrt(dx * dx + dy * dy) * focalLength(C.cam);
}
// List ranking by pointer jumping: w[k] >> 16 := the number of nodes that follow node k in the list `next` (n nodes, successor -1 at the
// tail).  A node's word holds (nodes skipped so far, the node reached) — one 32-bit word, so a reader always sees a consistent pair — and
// every round lets each node adopt its target's pair: the spans double, ceil(log2 n) rounds of a node per lane instead of a walk of n
// dependent reads.  (Updates in place: a target already updated in this round only makes the span longer.)
static_assert(MAX_ROWS < 0xffff, "list_rank packs a node index into 16 bits");
TC_FN void list_rank(uint32_t *w, const int32_t *next, int n) {
    for (int k = lane(); k < n; k += NL) {
        const int nx = next[k];
        w[k]         = nx >= 0 ? (1u << 16) | (uint32_t) nx : 0xffffu;
    }
    sync();
    for (int span = 1; span < n; span <<= 1) {
        for (int k = lane(); k < n; k += NL) {
            const uint32_t a = w[k], nx = a & 0xffffu;
            if (nx != 0xffffu) {
                const uint32_t b = w[nx];
                w[k]             = (((a >> 16) + (b >> 16)) << 16) | (b & 0xffffu);
            }
        }
        sync();
    }
}
// order_idx := the rows of f in container order (every row of a frame is a node of its list)
TC_FN int list_container_order(Stream &S, const Frame &f, Scratch &X) {
    const int n = f.n_rows;
    uint32_t *w = reinterpret_cast<uint32_t *>(X.lnk);
    list_rank(w, f.next, n);
    if (n > 0 && (f.head < 0 || (int) (w[f.head] >> 16) != n - 1)) { // (cannot happen: the list and the row count disagree) — the plain walk
        S.overflow |= OVF_INTERNAL;
        copy_n(X.next, f.next, n);
        int m = 0;
        for (int q = f.head; q >= 0 && m < MAX_ROWS; q = X.next[q]) S.order_idx[m++] = q;
        sync();
        return m;
    }
    for (int k = lane(); k < n; k += NL) S.order_idx[n - 1 - (int) (w[k] >> 16)] = k;
    sync();
    return n;
}
// Rows [n_old, f.n_rows) of frame f have just been written (f.n_rows already counts them; the container order covers the first n_old): they
// enter the container order one by one, in row order (bits/hashtable.h _M_insert_unique_node / _M_insert_bucket_begin / _M_rehash_aux, as
// order_insert_unique / order_rehash above) — keys, node list and buckets in the wave's scratch, written back when done
TC_FN void order_extend(Frame &f, int n_old, const uint32_t *buckets_after, Scratch &X) {
    const int n = f.n_rows;
    if (n <= n_old) return;
    int head = n_old ? f.head : -1, nb = n_old ? f.n_buckets : 1;
    u64 M    = n_old ? f.magic : 0;
    for (int k = lane(); k < n; k += NL) X.key[k] = f.row[k].id;
    for (int k = lane(); k < n_old; k += NL) X.next[k] = f.next[k];
    for (int b = lane(); b < nb; b += NL) X.bucket[b] = n_old ? f.bucket[b] : H_EMPTY;
    for (int k = n_old + 1 + lane(); k <= n; k += NL) X.want[k] = buckets_after[k]; // (one HBM load per insertion otherwise: ~1 us each)
    sync();
    // Round 5: the serial pass below is a chain of dependent LDS accesses per insertion; the 64-bit multiply-high of bucketOf sat on that
    // chain (once per insertion, once more for the old head, once per node of every rehash: ~0.23 ms for the 250 rows of a new frame).
    // Every bucket index it needs is known up front — row i enters under the bucket count buckets_after[i + 1], a rehash re-buckets the
    // nodes inserted so far under its new count — so they are computed a row per lane, and the chain keeps only the list surgery; the
    // bucket of the current head node is carried along (an insertion at the head moves it to the inserted row's bucket).
    for (int i = n_old + lane(); i < n; i += NL) {
        const int w = (int) X.want[i + 1];
        X.ibkt[i]   = (uint16_t) bucketOf(X.key[i], w, modMagic((u64) w));
    }
    sync();
    int head_bkt = head >= 0 ? bucketOf(X.key[head], nb, M) : 0; // bucket of the node `head` under nb (meaningful while head >= 0)
    for (int i = n_old; i < n; i++) {
        const int want = (int) X.want[i + 1];
        if (want != nb) { // _M_rehash_aux over the i nodes inserted so far
            const u64 M2 = modMagic((u64) want);
            for (int b = lane(); b < want; b += NL) X.tmp_bucket[b] = H_EMPTY;
            for (int p = lane(); p < i; p += NL) X.rbkt[p] = (uint16_t) bucketOf(X.key[p], want, M2);
            sync();
            int p = head;
            head  = -1;
            int bbegin_bkt = 0;
            while (p >= 0) {
                const int nx = X.next[p];
                const int b  = X.rbkt[p];
                if (X.tmp_bucket[b] == H_EMPTY) {
                    X.next[p]       = head;
                    head            = p;
                    X.tmp_bucket[b] = H_BEFORE_BEGIN;
                    if (X.next[p] >= 0) X.tmp_bucket[bbegin_bkt] = p;
                    bbegin_bkt = b;
                } else {
                    const int prev = X.tmp_bucket[b];
                    if (prev == H_BEFORE_BEGIN) {
                        X.next[p] = head;
                        head      = p;
                    } else {
                        X.next[p]    = X.next[prev];
                        X.next[prev] = p;
                    }
                }
                p = nx;
            }
            sync();
            for (int b = lane(); b < want; b += NL) X.bucket[b] = X.tmp_bucket[b];
            sync();
            nb       = want;
            M        = M2;
            head_bkt = bbegin_bkt; // (the bucket whose first node is the list head)
        }
        const int b = X.ibkt[i];
        if (X.bucket[b] != H_EMPTY) {
            const int prev = X.bucket[b];
            if (prev == H_BEFORE_BEGIN) { // the head's own bucket: the new node becomes the head, in the same bucket
                X.next[i] = head;
                head      = i;
            } else {
                X.next[i]    = X.next[prev];
                X.next[prev] = i;
            }
        } else {
            X.next[i] = head;
            if (head >= 0) X.bucket[head_bkt] = i; // the old head's bucket now begins after the new node
            head        = i;
            X.bucket[b] = H_BEFORE_BEGIN;
            head_bkt    = b;
        }
    }
    sync();
    for (int k = lane(); k < n; k += NL) f.next[k] = X.next[k];
    for (int b = lane(); b < nb; b += NL) f.bucket[b] = X.bucket[b];
    f.head      = head;
    f.n_buckets = nb;
    f.magic     = M;
    sync();
}
// The same container order WITHOUT the serial chain (round 5; VERDICT r4 item 4: "several lanes for the order insertions").  What
// _M_insert_bucket_begin does to the node list is the same for every insertion — a node whose bucket is empty goes to the head of the list,
// any other node to the front of its bucket's chain — and _M_rehash_aux re-enters the nodes in list order under the new bucket function by
// that very rule.  So after any run of insertions the list is the concatenation of the buckets' chains, chains ordered by the time their
// bucket received its first node (latest first), nodes inside a chain by their own time (latest first): a SORT of the events, not a walk.
// A phase = the rows entered under one bucket count (a rehash at its start re-enters the existing list, head first, as the phase's first
// events; a phase that continues a stored list without a rehash numbers the existing nodes tail first, which is the order they were
// entered in up to what the rule above can tell apart).  Per phase, a row per lane throughout: bucket of every event, per bucket the earliest
// event time (atomic min) and the chain size (atomic add), the chains' offsets by a suffix sum over time, the rank inside a chain by a walk of
// the bucket's short event list.  One new frame of 250 rows: six phases over 13 .. 250 events instead of 250 + 485 dependent steps.
// Results identical to order_extend (icgh_core_order_selftest against a real std::unordered_map, every engine test).
TC_FN void order_extend_parallel(Frame &f, int n_old, const uint32_t *buckets_after, Scratch &X) {
    const int n = f.n_rows;
    if (n <= n_old) return;
    int nb = n_old ? f.n_buckets : 1;
    for (int k = lane(); k < n; k += NL) X.key[k] = f.row[k].id;
    for (int k = lane(); k < n_old; k += NL) X.next[k] = f.next[k];
    for (int k = n_old + 1 + lane(); k <= n; k += NL) X.want[k] = buckets_after[k];
    sync();
    int cur = 0, m = 0; // list order so far: X.ord[cur][0 .. m), head first
    if (n_old) {       // the stored list as an array: a node's place is n_old - 1 - (nodes that follow it)
        uint32_t *w = reinterpret_cast<uint32_t *>(X.lnk);
        list_rank(w, X.next, n_old);
        for (int k = lane(); k < n_old; k += NL) X.ord[cur][n_old - 1 - (int) (w[k] >> 16)] = (uint16_t) k;
        m = n_old;
        sync();
    }
    bool continued = n_old > 0; // the stored list continues without a rehash (first phase only)
    int ra         = n_old;
    while (ra < n) {
        const int want = (int) X.want[ra + 1];
        if (want != nb) continued = false; // _M_rehash_aux before row ra enters: the existing nodes are re-entered head first
        nb = want;
        int rb = ra + 1; // rows [ra, rb) enter under nb: rb = the first row past ra that meets another bucket count (a chunk of rows per step)
        for (;;) {
            const int k   = rb + lane();
            const u64 end = ballot(k >= n || (int) X.want[k + 1] != nb);
            if (end) {
                rb += first_lane(end);
                break;
            }
            rb += NL;
        }
        const u64 M = modMagic((u64) nb);
        const int E = m + (rb - ra); // events of the phase; event e < m: node ord[e]; else row ra + (e - m); time: see below
        uint32_t *bfirst = reinterpret_cast<uint32_t *>(X.tmp_bucket), *bcnt = reinterpret_cast<uint32_t *>(X.bucket);
        for (int b = lane(); b < nb; b += NL) bfirst[b] = 0xffffffffu, bcnt[b] = 0, X.bhead[b] = -1;
        for (int t = lane(); t <= E; t += NL) X.tsum[t] = 0;
        sync();
        for (int e = lane(); e < E; e += NL) {
            const int node = e < m ? (int) X.ord[cur][e] : ra + (e - m);
            const int t    = (e < m && continued) ? m - 1 - e : e;
            const int b    = bucketOf(X.key[node], nb, M);
            X.rbkt[e]      = (uint16_t) b;
            X.ibkt[node]   = (uint16_t) b;
            lds_min(&bfirst[b], (uint32_t) t);
            lds_add(&bcnt[b], 1u);
            X.lnk[e] = lds_exch(&X.bhead[b], e);
        }
        sync();
        // tsum[t] := size of the chain whose bucket received its first node at time t (0 for the other times)
        for (int e = lane(); e < E; e += NL) {
            const int t = (e < m && continued) ? m - 1 - e : e;
            const int b = X.rbkt[e];
            if (bfirst[b] == (uint32_t) t) X.tsum[t] = bcnt[b];
        }
        sync();
        // tsum[t] := number of nodes in chains that started LATER than t (they precede the chain that started at t): suffix sums, a
        // chunk of NL times per step from the top
        {
            uint32_t carry = 0;
            for (int hi = E; hi > 0; hi -= NL) {
                const int t      = hi - 1 - lane(); // descending times across the lanes
                const uint32_t v = t >= 0 ? X.tsum[t] : 0u;
                const uint32_t inc = wave_scan_incl(v); // sum over times >= t inside the chunk
                if (t >= 0) X.tsum[t] = carry + inc - v;
                uint32_t tot = inc; // chunk total = the inclusive sum of the chunk's last lane (or the one value on the host)
#if defined(__HIP_DEVICE_COMPILE__)
                tot = (uint32_t) __shfl((int) inc, 63, 64);
#endif
                carry += tot;
                sync();
            }
        }
        sync();
        const int nxt = cur ^ 1;
        for (int e = lane(); e < E; e += NL) {
            const int node = e < m ? (int) X.ord[cur][e] : ra + (e - m);
            const int t    = (e < m && continued) ? m - 1 - e : e;
            const int b    = X.rbkt[e];
            int rank       = 0; // events of the same bucket that entered later (they sit in front)
            for (int o = X.bhead[b]; o >= 0; o = X.lnk[o]) {
                const int to = (o < m && continued) ? m - 1 - o : o;
                rank += to > t ? 1 : 0;
            }
            X.ord[nxt][(int) X.tsum[bfirst[b]] + rank] = (uint16_t) node;
        }
        sync();
        cur = nxt, m = E, ra = rb;
        continued = false;
    }
    // node list and bucket heads of the final order
    for (int b = lane(); b < nb; b += NL) X.bucket[b] = H_EMPTY;
    sync();
    for (int p = lane(); p < m; p += NL) {
        const int node = X.ord[cur][p];
        X.next[node]   = p + 1 < m ? (int) X.ord[cur][p + 1] : -1;
        const int b    = X.ibkt[node];
        if (p == 0)
            X.bucket[b] = H_BEFORE_BEGIN;
        else if ((int) X.ibkt[X.ord[cur][p - 1]] != b)
            X.bucket[b] = (int) X.ord[cur][p - 1];
    }
    sync();
    for (int k = lane(); k < n; k += NL) f.next[k] = X.next[k];
    for (int b = lane(); b < nb; b += NL) f.bucket[b] = X.bucket[b];
    f.head      = m > 0 ? (int) X.ord[cur][0] : -1;
    f.n_buckets = nb;
    f.magic     = modMagic((u64) nb);
    sync();
}
// rows [n_old, f.n_rows) enter the container order: the sort for batches that are worth it (a new frame's rows, an extension across a
// rehash of a full frame), the serial list surgery for the handful of rows a triangulation adds
TC_FN void order_extend_auto(Frame &f, int n_old, const uint32_t *buckets_after, Scratch &X) {
    const int n = f.n_rows;
    if (n <= n_old) return;
    const bool rehash = (int) buckets_after[n] != (n_old ? f.n_buckets : 1);
    if (n - n_old >= 32 || (rehash && n_old >= 48))
        order_extend_parallel(f, n_old, buckets_after, X);
    else
        order_extend(f, n_old, buckets_after, X);
}
// the sum of a parallax average: terms in the order the reference adds them, added one by one.  The terms (X.key as doubles) and their
// validity (X.next) were filled in parallel into the wave's scratch: the sequential pass reads LDS, not HBM
TC_FN double key_as_double(u64 v) {
    double d;
    memcpy(&d, &v, sizeof d);
    return d;
}
TC_FN u64 double_as_key(double d) {
    u64 v;
    memcpy(&v, &d, sizeof v);
    return v;
}
// the mean of the flagged terms, added one by one in list order as the reference does (:896-903, :915-920).  The order of the additions is the
// result; what need not be serial is fetching the terms: a chunk is loaded a term per lane, then read lane by lane out of the registers.
TC_FN int sum_parallax_terms(const Scratch &X, int n, double &parallax) {
    parallax   = 0;
    int counts = 0;
    for (int base = 0; base < n; base += NL) {
        const int k    = base + lane();
        const bool on  = k < n && X.next[k] != 0;
        const double v = on ? key_as_double(X.key[k]) : 0.0;
        u64 m          = ballot(on);
        counts += popc(m);
        while (m) {
            const int l = first_lane(m);
            parallax += lane_get(v, l);
            m &= m - 1;
        }
    }
    if (counts != 0) parallax /= counts;
    return counts;
}
TC_FN int parallax_from_reference_mappoints(Stream &S, const Cfg &C, double &parallax, Scratch &X) { // :873-905
    const Frame &fc = S.frame[S.cur];
    const Frame &fr = S.frame[S.ref];
    double R10[9];
    mat_mul_t(fc.pose.R, fr.pose.R, R10);
    const double focal = focalLength(C.cam);
    const int nq       = list_container_order(S, fr, X);
    TC_MARK(26);
    // four chunks of rows at a time, level by level: order -> row of the reference frame -> its map point -> the row the map point was
    // last seen in.  Each level's loads are issued for all four chunks before the first is used (one memory round trip per level, not per
    // level and chunk); the values and the order of the arithmetic are those of the row-by-row form.
    constexpr int U = 4;
    const int cur       = S.cur;
    const uint32_t cgen = fc.gen;
    for (int base = 0; base < nq; base += U * NL) {
        int kk[U], idx[U];
        TC_UNROLL for (int u = 0; u < U; u++) {
            kk[u]  = base + u * NL + lane();
            idx[u] = kk[u] < nq ? S.order_idx[kk[u]] : -1;
        }
        uint32_t mp[U], mpgen[U];
        double pcx[U], pcy[U];
        TC_UNROLL for (int u = 0; u < U; u++) {
            const Row &r0 = fr.row[idx[u] >= 0 ? idx[u] : 0];
            mp[u] = r0.mp, mpgen[u] = r0.mpgen, pcx[u] = r0.pcx, pcy[u] = r0.pcy;
        }
        bool ok[U];
        LastObs lo[U];
        TC_UNROLL for (int u = 0; u < U; u++) {
            const MpHot &h = S.hot[idx[u] >= 0 ? mp[u] : 0];
            ok[u] = idx[u] >= 0 && h.live && h.gen == mpgen[u] && !h.outlier; // getMapPoint() && !isOutlier()
            lo[u] = h.last;                                                     // observations().back().lock()
            ok[u] = ok[u] && lo[u].frame == cur && lo[u].gen == cgen;         // feat && feat->getFrame() == frame_cur_
        }
        uint8_t out1[U];
        double x1[U], y1[U];
        TC_UNROLL for (int u = 0; u < U; u++) {
            const Row &r1 = fc.row[ok[u] ? lo[u].row : 0];
            out1[u] = r1.outlier, x1[u] = r1.pcx, y1[u] = r1.pcy;
        }
        TC_UNROLL for (int u = 0; u < U; u++) {
            if (kk[u] >= nq) continue;
            const bool good = ok[u] && !out1[u]; // :884
            double term     = 0;
            if (good) {
                const double x = R10[0] * pcx[u] + R10[1] * pcy[u] + R10[2] * 1.0, y = R10[3] * pcx[u] + R10[4] * pcy[u] + R10[5] * 1.0;
                const double dx = x - x1[u], dy = y - y1[u];
                term            = tc_sqrt(dx * dx + dy * dy) * focal;
            }
            X.next[kk[u]] = good ? 1 : 0;
            X.key[kk[u]]  = double_as_key(term);
        }
    }
    sync();
    TC_MARK(27);
    return sum_parallax_terms(X, nq, parallax);
}
TC_FN int parallax_from_reference_keypoints(Stream &S, const Cfg &C, const P2f *ref, const P2f *cur, double &parallax, Scratch &X) { // :907-922
    double R10[9];
    mat_mul_t(S.frame[S.cur].pose.R, S.frame[S.ref].pose.R, R10);
    const int n = S.n_ref_frame;
    for (int k = lane(); k < n; k += NL) {
        const bool ok = S.pts2d_ref_frame[k] == S.ref;
        X.next[k]     = ok ? 1 : 0;
        X.key[k]      = double_as_key(ok ? keypoint_parallax(C, ref[k], cur[k], R10) : 0.0);
    }
    sync();
    return sum_parallax_terms(X, n, parallax);
}
TC_FN void clear_candidates(Stream &S) {
    S.n_new = S.n_ref = S.n_ref_undis = S.n_new_undis = S.n_ref_frame = S.n_vel_ref = S.n_cand_lk = 0;
}
TC_FN bool do_reset_tracking(Stream &S) { // :317-329
    if (!S.frame[S.cur].n_rows) {
        S.isinitializing = 1;
        S.ref            = S.cur;
        clear_candidates(S);
        return true;
    }
    return false;
}
TC_FN int check_keyframe_state(Stream &S, const Cfg &C) { // :263-307
    int keyframe_state = KEYFRAME_NONE;
    const double dt    = S.frame[S.cur].stamp - S.frame[S.last_keyframe].stamp;
    if (dt < 0.08 /*TRACK_MIN_INTERVAl*/) return keyframe_state;
    const double parallax = (S.parallax_map * S.parallax_map_counts + S.parallax_ref * S.parallax_ref_counts) /
                            (S.parallax_map_counts + S.parallax_ref_counts);
    if (parallax > C.track_min_parallax) {
        keyframe_state = S.is_window_full ? KEYFRAME_REMOVE_OLDEST : KEYFRAME_NORMAL;
    } else if (dt > C.track_max_interval) {
        keyframe_state = KEYFRAME_REMOVE_SECOND_NEW;
    }
    if (keyframe_state != KEYFRAME_NONE) {
        S.last_keyframe = S.cur;
        for (int k = lane(); k < S.n_tracked; k += NL) { // (the tracked map points are distinct: independent increments)
            const MpRef m = S.tracked_mappoint[k];
            if (mp_valid(S, m.i, m.g)) S.hot[m.i].used++;
        }
        sync();
        const Pose &pc = S.frame[S.cur].pose, &pr = S.frame[S.ref].pose;
        const double dx = pc.t[0] - pr.t[0], dy = pc.t[1] - pr.t[1], dz = pc.t[2] - pr.t[2];
        double R[9];
        mat_mul_t(pc.R, pr.R, R);
        const double pitch = atan(-R[6] / tc_sqrt(R[7] * R[7] + R[8] * R[8])); // :335-341
        S.log_data[0] = S.frame[S.cur].stamp, S.log_data[1] = dt, S.log_data[2] = parallax;
        S.log_data[3] = tc_sqrt(dx * dx + dy * dy + dz * dz); // :331-333
        S.log_data[4] = tc_fabs(pitch * (180.0 / 3.14159265358979323846));
        S.log_valid   = 1;
    }
    return keyframe_state;
}

TC_FN void finish(Stream &S, int st) {
    S.result = st;
    S.done   = 1;
}

// ---- featuresDetection (:576-688) ------------------------------------------------------------------------------------------------------
TC_FN bool queue_detection(Stream &S, const Cfg &C, Io &io, int frame, bool ismask, Scratch &X) {
    S.det_job        = -1;
    const Frame &f   = S.frame[frame];
    const int num_features = f.n_rows + S.n_ref; // :579
    if (num_features > (C.track_max_features - 5)) return false; // :580
    uint32_t *features_cnts = X.tsum; // (a histogram in the wave's scratch memory: a point per lane, one atomic add each)
    for (int k = lane(); k < C.block_cnts; k += NL) features_cnts[k] = 0;
    sync();
    const int total = f.n_rows + S.n_new;
    for (int q = lane(); q < total; q += NL) {
        const P2f p   = q < f.n_rows ? f.row[q].kp : S.pts2d_new[q - f.n_rows];
        const int col = (int) (p.x / (float) C.block_w); // :598
        const int row = (int) (p.y / (float) C.block_h);
        // hazard H5 (unclamped column of an undistorted key point), reproduced as in tracking_hip.cc: the index may name another block or none
        const long idx = (long) row * C.block_cols + col;
        if (idx >= 0 && idx < (long) C.block_cnts) lds_add(&features_cnts[idx], 1u);
    }
    sync();
    S.det_job     = 0;
    S.det_ismask  = ismask ? 1 : 0;
    S.det_frame   = frame;
    *io.det_slot  = f.slot;
    int nm        = 0;
    if (ismask) { // :610-620 (a union of discs: the order of the points is immaterial)
        const Frame &fc = S.frame[S.cur];
        nm              = fc.n_rows + S.n_new;
        if (nm > MAX_ROWS) nm = MAX_ROWS;
        for (int q = lane(); q < nm; q += NL) io.det_mask_pts[q] = q < fc.n_rows ? fc.row[q].kp : S.pts2d_new[q - fc.n_rows];
    }
    *io.det_mask_count = nm;
    for (int k = lane(); k < C.block_cnts; k += NL) io.det_quota[k] = C.max_block_features - (int) features_cnts[k]; // :629
    sync();
    return true;
}
TC_FN void integrate_detection(Stream &S, const Cfg &C, const Io &io) { // :659-685
    if (!S.det_ismask) clear_candidates(S);
    int n = *io.det_count;
    if (S.n_ref + n > MAX_ROWS || S.n_new + n > MAX_ROWS) {
        S.overflow |= OVF_ROWS;
        n = 0;
    }
    const int r0 = S.n_ref, n0 = S.n_new, ru0 = S.n_ref_undis, nu0 = S.n_new_undis, f0 = S.n_ref_frame, v0 = S.n_vel_ref;
    for (int i = lane(); i < n; i += NL) {
        const P2f p = io.det_out[i];
        const P2f u = undistortPoint(C.cam, p); // the one undistortion a detected corner ever needs
        S.pts2d_ref[r0 + i]        = p;
        S.pts2d_new[n0 + i]        = p;
        S.pts2d_ref_undis[ru0 + i] = u;
        S.pts2d_new_undis[nu0 + i] = u;
        S.pts2d_ref_frame[f0 + i]  = S.det_frame;
        S.velocity_ref[v0 + i][0] = 0, S.velocity_ref[v0 + i][1] = 0;
    }
    S.n_ref = r0 + n, S.n_new = n0 + n, S.n_ref_undis = ru0 + n, S.n_new_undis = nu0 + n, S.n_ref_frame = f0 + n, S.n_vel_ref = v0 + n;
    // cand_lk_idx_.resize(pts2d_new_.size(), -1): a list that lost its alignment is padded / cut (hints are hints)
    for (int k = S.n_cand_lk + lane(); k < S.n_new; k += NL) S.cand_lk_idx[k] = -1;
    S.n_cand_lk = S.n_new;
    S.det_job   = -1;
    S.det_frame = -1;
    sync();
}

// ---- trackMappoint (:351-455) ------------------------------------------------------------------------------------------------------------
TC_FN void queue_track_mappoint(Stream &S, const Cfg &C, Io &io, Scratch &X) {
    S.n_matched     = 0;
    const Frame &fp = S.frame[S.pre];
    const Pose pose_cur = S.frame[S.cur].pose;
    const int cur_slot  = S.frame[S.cur].slot;
    const int nq    = list_container_order(S, fp, X);
    TC_MARK(14);
    int n           = 0;
    // rows in container order, four chunks at a time and level by level (order -> row -> its map point: a memory round trip per level, not per
    // level and chunk); the valid ones are appended in that order
    constexpr int U   = 4;
    const int pslot   = fp.slot;
    for (int base = 0; base < nq; base += U * NL) {
        int kk[U], idx[U];
        TC_UNROLL for (int u = 0; u < U; u++) {
            kk[u]  = base + u * NL + lane();
            idx[u] = kk[u] < nq ? S.order_idx[kk[u]] : -1;
        }
        Row r[U];
        TC_UNROLL for (int u = 0; u < U; u++) r[u] = fp.row[idx[u] >= 0 ? idx[u] : 0];
        bool valid[U];
        double pos[U][3];
        TC_UNROLL for (int u = 0; u < U; u++) {
            const MpHot &h = S.hot[idx[u] >= 0 ? r[u].mp : 0];
            valid[u] = idx[u] >= 0 && h.live && h.gen == r[u].mpgen && !h.outlier; // mappoint && !mappoint->isOutlier() (:360)
            pos[u][0] = h.pos[0], pos[u][1] = h.pos[1], pos[u][2] = h.pos[2];
        }
        TC_UNROLL for (int u = 0; u < U; u++) {
            P2f pp;
            pp.x = pp.y = 0;
            if (valid[u]) {
                pp = world2pixel(C.cam, pos[u], pose_cur); // INS-aided prediction :367
                distortPoint(C.cam, pp);                   // :378
            }
            const u64 m   = ballot(valid[u]);
            const int at  = n + popc(m & lanes_below());
            if (valid[u]) {
                S.tm_pc[at][0] = r[u].pcx, S.tm_pc[at][1] = r[u].pcy;
                io.lk_prev_slot[at] = pslot;
                io.lk_next_slot[at] = cur_slot;
                io.lk_prev[at]      = r[u].kpd;
                io.lk_guess[at]     = pp;
                MpRef mr;
                mr.i = r[u].mp, mr.g = r[u].mpgen;
                S.mappoint_matched[at] = mr;
            }
            n += popc(m);
        }
    }
    S.n_matched    = n;
    S.lk_map_begin = 0;
    S.lk_map_n     = n;
    *io.lk_count   = n;
    sync();
    TC_MARK(15);
}
TC_FN bool finish_track_mappoint(Stream &S, const Cfg &C, const Io &io, const uint32_t *buckets_after, Scratch &X) {
    if (S.lk_map_n == 0) return false;
    const int n           = S.lk_map_n;
    const uint8_t *status = io.lk_status + S.lk_map_begin;
    const P2f *out        = io.lk_out + S.lk_map_begin;
    const P2f *undis      = io.lk_undist + S.lk_map_begin;
    int kept = 0;
    for (int base = 0; base < n; base += NL) {
        const int k = base + lane();
        kept += popc(ballot(k < n && status[k]));
    }
    if (kept == 0) { // :410-419
        S.parallax_map        = 0;
        S.parallax_map_counts = 0;
        return false;
    }
    TC_MARK(21);
    Frame &fc = S.frame[S.cur];
    frame_clear_rows(fc); // :426
    if (kept > MAX_ROWS) { // (cannot happen: n <= MAX_ROWS)
        S.overflow |= OVF_ROWS;
        return false;
    }
    const double dt     = fc.stamp - S.frame[S.pre].stamp;
    const uint32_t cgen = fc.gen;
    int r0 = 0;
    // reduceVector (:404-408) and the feature loop (:430-444): the rows of the kept points, in order — four chunks of points at a time, the
    // LK results and the matched map points of all four loaded before the map points' records are (two memory round trips per four chunks)
    constexpr int U = 4;
    const int curh  = S.cur;
    for (int base = 0; base < n; base += U * NL) {
        int kk[U];
        bool keep[U];
        MpRef mref[U];
        P2f und[U], o2[U];
        double pc0[U][2];
        TC_UNROLL for (int u = 0; u < U; u++) {
            kk[u]        = base + u * NL + lane();
            const int k  = kk[u] < n ? kk[u] : 0;
            keep[u]      = kk[u] < n && status[k];
            mref[u]      = S.mappoint_matched[k];
            und[u]       = undis[k];
            o2[u]        = out[k];
            pc0[u][0] = S.tm_pc[k][0], pc0[u][1] = S.tm_pc[k][1];
        }
        u64 hid[U];
        uint32_t hgen[U];
        TC_UNROLL for (int u = 0; u < U; u++) {
            const MpHot &h = S.hot[keep[u] ? mref[u].i : 0];
            hid[u] = h.id, hgen[u] = h.gen;
        }
        TC_UNROLL for (int u = 0; u < U; u++) {
            const u64 mm = ballot(keep[u]);
            if (keep[u]) {
                const int k   = kk[u];
                const int row = r0 + popc(mm & lanes_below());
                const MpRef m = mref[u];
                double pcx, pcy;
                pixel2cam(C.cam, und[u], pcx, pcy);
                Row r;
                r.id      = hid[u];
                r.mp      = m.i;
                r.mpgen   = hgen[u];
                r.kp      = und[u];
                r.kpd     = o2[u];
                r.vel[0]  = (pcx - pc0[u][0]) / dt; // (pixel2cam(cur) - pixel2cam(pre)) / dt (:434)
                r.vel[1]  = (pcy - pc0[u][1]) / dt;
                r.pcx     = pcx;
                r.pcy     = pcy;
                r.lk_idx  = io.lk_base + S.lk_map_begin + k;
                r.type    = (int8_t) FEATURE_MATCHED;
                r.outlier = 0;
                r.pad_[0] = r.pad_[1] = 0;
                fc.row[row] = r;
                S.hot[m.i].observed++; // addObservation (mappoint.cc:58-62); the matched map points are distinct
                LastObs lo;
                lo.frame = curh, lo.gen = cgen, lo.row = row;
                S.hot[m.i].last          = lo;
                S.tracked_mappoint[row] = m;
            }
            r0 += popc(mm);
        }
    }
    S.n_tracked = kept;
    fc.n_rows   = kept;
    sync();
    TC_MARK(22);
    order_extend_auto(fc, 0, buckets_after, X); // the ids of the previous frame's rows are distinct keys
    TC_MARK(23);
    S.parallax_map_counts = parallax_from_reference_mappoints(S, C, S.parallax_map, X); // :450
    TC_MARK(24);
    return true;
}

// ---- trackReferenceFrame (:457-574) ----------------------------------------------------------------------------------------------------
TC_FN void queue_track_reference(Stream &S, const Cfg &C, Io &io) {
    S.lk_ref_begin = *io.lk_count;
    S.lk_ref_n     = 0;
    if (S.n_ref == 0) return; // :459-462
    const Frame &fc = S.frame[S.cur], &fp = S.frame[S.pre];
    double r_cur_pre[9];
    mat_mul_t(fc.pose.R, fp.pose.R, r_cur_pre); // :465
    const int at = S.lk_ref_begin;
    if (at + S.n_new > MAX_ROWS) {
        S.overflow |= OVF_ROWS;
        return;
    }
    const int nu = S.n_new_undis;
    for (int k = lane(); k < nu; k += NL) { // :469 (carried), :472-479
        double x, y;
        pixel2cam(C.cam, S.pts2d_new_undis[k], x, y);
        const double X = r_cur_pre[0] * x + r_cur_pre[1] * y + r_cur_pre[2] * 1.0, Y = r_cur_pre[3] * x + r_cur_pre[4] * y + r_cur_pre[5] * 1.0,
                     Z = r_cur_pre[6] * x + r_cur_pre[7] * y + r_cur_pre[8] * 1.0;
        S.pts2d_cur[k] = distortCameraPoint(C.cam, X, Y, Z);
    }
    S.n_cur = nu;
    sync();
    S.lk_ref_n = S.n_new;
    const int pslot = fp.slot, cslot = fc.slot;
    for (int k = lane(); k < S.lk_ref_n; k += NL) {
        io.lk_prev_slot[at + k] = pslot;
        io.lk_next_slot[at + k] = cslot;
        io.lk_prev[at + k]      = S.pts2d_new[k];
        io.lk_guess[at + k]     = S.pts2d_cur[k];
    }
    *io.lk_count = at + S.lk_ref_n;
    sync();
}
TC_FN bool mid_track_reference(Stream &S, const Cfg &C, Io &io, Scratch &X) {
    S.rs_set      = -1;
    *io.rs_count  = 0;
    if (S.lk_ref_n == 0) return false;
    const int n = S.lk_ref_n;
    for (int k = lane(); k < n; k += NL) {
        S.status[k]      = io.lk_status[S.lk_ref_begin + k];
        S.pts2d_cur[k]   = io.lk_out[S.lk_ref_begin + k];
        S.scratch_a[k]   = io.lk_undist[S.lk_ref_begin + k];
        S.cand_lk_idx[k] = io.lk_base + S.lk_ref_begin + k;
    }
    S.n_cur = n;
    sync();
    TC_MARK(60);
    // reduceVector (:507-511): every list by the LK status
    auto c_lk = compact(S.cand_lk_idx, n);
    auto c_ref = compact(S.pts2d_ref, S.n_ref);
    auto c_cur = compact(S.pts2d_cur, S.n_cur);
    auto c_new = compact(S.pts2d_new, S.n_new);
    auto c_rf = compact(S.pts2d_ref_frame, S.n_ref_frame);
    auto c_vr = compact2(S.velocity_ref, S.n_vel_ref);
    auto c_a = compact(S.scratch_a, n);
    auto c_ru = compact(S.pts2d_ref_undis, S.n_ref_undis);
    auto c_nu = compact(S.pts2d_new_undis, S.n_new_undis);
    reduce_vectors(S.status, c_lk, c_ref, c_cur, c_new, c_rf, c_vr, c_a, c_ru, c_nu);
    S.n_cand_lk = c_lk.kept, S.n_ref = c_ref.kept, S.n_cur = c_cur.kept, S.n_new = c_new.kept, S.n_ref_frame = c_rf.kept, S.n_vel_ref = c_vr.kept;
    const int n_a = c_a.kept;
    S.n_ref_undis = c_ru.kept, S.n_new_undis = c_nu.kept;
    TC_MARK(61);
    if (S.n_ref == 0) return false; // :513-517 (tr_cur_undis_ keeps what it held, as in the table)
    copy_n(S.tr_cur_undis, S.scratch_a, n_a);
    S.n_tr_cur_undis = n_a;
    copy_n(S.tr_new_undis, S.pts2d_new_undis, S.n_new_undis); // :520-524 (carried)
    S.n_tr_new_undis = S.n_new_undis;

    // :527-539
    const Frame &fc   = S.frame[S.cur];
    const u64 ref_fid = S.frame[S.ref].fid;
    const double dt   = fc.stamp - S.frame[S.pre].stamp;
    for (int k = lane(); k < S.n_tr_cur_undis; k += NL) {
        double x1, y1, x0, y0;
        pixel2cam(C.cam, S.tr_cur_undis[k], x1, y1);
        pixel2cam(C.cam, S.tr_new_undis[k], x0, y0);
        const double vx = (x1 - x0) / dt, vy = (y1 - y0) / dt;
        S.velocity_cur[k][0] = vx, S.velocity_cur[k][1] = vy;
        if (S.frame[S.pts2d_ref_frame[k]].fid > ref_fid) S.velocity_ref[k][0] = vx, S.velocity_ref[k][1] = vy;
    }
    S.n_vel_cur = S.n_tr_cur_undis;
    sync();
    TC_MARK(62);
    S.parallax_ref_counts = parallax_from_reference_keypoints(S, C, S.pts2d_ref_undis, S.tr_cur_undis, S.parallax_ref, X); // :542-544
    TC_MARK(63);

    if (S.n_cur >= 15) { // :547-548
        S.rs_set = 0;
        const int m = S.n_tr_new_undis;
        for (int k = lane(); k < m; k += NL) {
            io.rs_p1[k] = S.tr_new_undis[k];
            io.rs_p2[k] = S.tr_cur_undis[k];
        }
        *io.rs_count = m;
        sync();
    }
    return true;
}
TC_FN bool finish_track_reference(Stream &S, const Io &io) {
    if (S.rs_set >= 0) { // :550-554
        const uint8_t *mask = io.rs_mask;
        const int m         = S.n_tr_new_undis; // (the set's size)
        for (int k = lane(); k < m; k += NL) S.status[k] = mask[k];
        sync();
        auto c_ref = compact(S.pts2d_ref, S.n_ref);
        auto c_cur = compact(S.pts2d_cur, S.n_cur);
        auto c_rf = compact(S.pts2d_ref_frame, S.n_ref_frame);
        auto c_vc = compact2(S.velocity_cur, S.n_vel_cur);
        auto c_vr = compact2(S.velocity_ref, S.n_vel_ref);
        auto c_ru = compact(S.pts2d_ref_undis, S.n_ref_undis);
        auto c_cu = compact(S.tr_cur_undis, S.n_tr_cur_undis);
        auto c_lk = compact(S.cand_lk_idx, S.n_cand_lk);
        reduce_vectors(S.status, c_ref, c_cur, c_rf, c_vc, c_vr, c_ru, c_cu, c_lk);
        S.n_ref = c_ref.kept, S.n_cur = c_cur.kept, S.n_ref_frame = c_rf.kept, S.n_vel_cur = c_vc.kept, S.n_vel_ref = c_vr.kept;
        S.n_ref_undis = c_ru.kept, S.n_tr_cur_undis = c_cu.kept, S.n_cand_lk = c_lk.kept;
        S.rs_set         = -1;
    }
    if (S.n_cur == 0) return false; // :557-561
    copy_n(S.pts2d_new, S.pts2d_cur, S.n_cur); // :569
    S.n_new = S.n_cur;
    copy_n(S.pts2d_new_undis, S.tr_cur_undis, S.n_tr_cur_undis);
    S.n_new_undis = S.n_tr_cur_undis;
    return S.n_new != 0;
}

// ---- triangulation (:690-798) ----------------------------------------------------------------------------------------------------------
TC_FN void pose2Tcw12(const Pose &pose, double *t12) { // :851-859, upper 3 x 4 block row-major
    const double *R = pose.R;
    // Rt = R^T; t = Rt * pose.t
    const double t0 = R[0] * pose.t[0] + R[3] * pose.t[1] + R[6] * pose.t[2];
    const double t1 = R[1] * pose.t[0] + R[4] * pose.t[1] + R[7] * pose.t[2];
    const double t2 = R[2] * pose.t[0] + R[5] * pose.t[1] + R[8] * pose.t[2];
    t12[0] = R[0], t12[1] = R[3], t12[2] = R[6], t12[3] = -t0;
    t12[4] = R[1], t12[5] = R[4], t12[6] = R[7], t12[7] = -t1;
    t12[8] = R[2], t12[9] = R[5], t12[10] = R[8], t12[11] = -t2;
}
TC_FN bool queue_triangulation(Stream &S, const Cfg &C, Io &io, Scratch &X) {
    S.tri_queued   = 0;
    *io.tri_count  = 0;
    *io.tri_n_tcw  = 0;
    if (S.n_cur == 0) return false; // :692-694
    S.tri_queued     = 1;
    const Pose pose1 = S.frame[S.cur].pose;
    if (S.n_tr_cur_undis != S.n_cur) { // no reference tracking ran this frame: derive them
        for (int k = lane(); k < S.n_cur; k += NL) S.tr_cur_undis[k] = undistortPoint(C.cam, S.pts2d_cur[k]);
        S.n_tr_cur_undis = S.n_cur;
        sync();
    }
    if (S.n_ref_undis != S.n_ref) {
        for (int k = lane(); k < S.n_ref; k += NL) S.pts2d_ref_undis[k] = undistortPoint(C.cam, S.pts2d_ref[k]);
        S.n_ref_undis = S.n_ref;
        sync();
    }
    copy_n(S.tri_ref_undis, S.pts2d_ref_undis, S.n_ref_undis); // :712-713 (carried)
    S.n_tri_ref_undis = S.n_ref_undis;
    copy_n(S.tri_cur_undis, S.tr_cur_undis, S.n_tr_cur_undis);
    S.n_tri_cur_undis = S.n_tr_cur_undis;
    for (int k = lane(); k < S.n_cur; k += NL) S.tri_status[k] = 0;
    S.n_tri_status = S.n_cur;
    sync();
    S.n_tri_index  = 0;
    S.tri_begin    = 0;
    TC_MARK(33);

    int n_tcw = 0, n_tri = 0;
    const int T_cur = n_tcw;
    pose2Tcw12(pose1, io.tri_Tcw + 12 * n_tcw);
    n_tcw++;
    // pass 1 (parallel): what happens to candidate k — 0 re-anchored (:723-730), 1 dropped (:733-737), 2 kept for later (:741-746),
    // 3 triangulated — and, for 3, its two normalized points
    const u64 ref_fid = S.frame[S.ref].fid;
    for (int k = lane(); k < S.n_cur; k += NL) {
        const int frame_ref = S.pts2d_ref_frame[k];
        const Frame &fr     = S.frame[frame_ref];
        int kind;
        if (fr.fid > ref_fid) { // feature added after the reference keyframe: re-anchor
            S.pts2d_ref_frame[k] = S.cur;
            S.pts2d_ref[k]       = S.pts2d_cur[k];
            S.pts2d_ref_undis[k] = S.tri_cur_undis[k];
            S.tri_status[k]      = 1;
            kind                 = 0;
        } else if (S.n_map_kf == C.window_size && !map_is_keyframe_in_map(S, frame_ref)) {
            S.tri_status[k] = 0;
            kind            = 1;
        } else {
            double R10[9];
            mat_mul_t(pose1.R, fr.pose.R, R10); // (pose1.R^T * pose0.R)
            const double parallax = keypoint_parallax(C, S.tri_ref_undis[k], S.tri_cur_undis[k], R10); // :741
            if (parallax < 10.0 /*TRACK_MIN_PARALLAX*/) {
                S.tri_status[k] = 1;
                kind            = 2;
            } else {
                kind = 3;
                pixel2cam(C.cam, S.tri_ref_undis[k], S.tri_tmp[k][0], S.tri_tmp[k][1]); // :750-751
                pixel2cam(C.cam, S.tri_cur_undis[k], S.tri_tmp[k][2], S.tri_tmp[k][3]);
            }
        }
        X.next[k] = kind;
    }
    sync();
    TC_MARK(34);
    // pass 2 (a chunk of candidates per step): camera matrices of the distinct reference frames in order of first appearance, the
    // triangulation list by rank.  The one-by-one loop looks a reference frame up in a table of the first 8 distinct ones and enters it when
    // absent: per chunk the lanes are served leader first — a frame in the table (or just entered) serves all its lanes at once, a frame the
    // full table cannot take is handled lane by lane, as the loop would (a fresh camera matrix per occurrence)
    int T_frame[8], T_index[8], n_T = 0;
    for (int base = 0; base < S.n_cur; base += NL) {
        const int k    = base + lane();
        const bool tri = k < S.n_cur && X.next[k] == 3;
        const int fr   = tri ? S.pts2d_ref_frame[k] : -1;
        const u64 m3   = ballot(tri);
        u64 todo       = m3;
        int T0         = -1;
        while (todo) {
            const int leader = first_lane(todo);
            const int h      = lane_get(fr, leader);
            int t0 = -1;
            for (int q = 0; q < n_T; q++)
                if (T_frame[q] == h) t0 = T_index[q];
            u64 grp = ballot(tri && fr == h) & todo;
            if (t0 < 0) {
                if (n_tcw >= MAX_TCW) {
                    S.overflow |= OVF_TCW;
                    t0 = 0;
                } else {
                    t0 = n_tcw;
                    pose2Tcw12(S.frame[h].pose, io.tri_Tcw + 12 * n_tcw);
                    n_tcw++;
                }
                if (n_T < 8) {
                    T_frame[n_T] = h, T_index[n_T] = t0, n_T++;
                } else {
                    grp = 1ull << leader;
                }
            }
            if ((grp >> lane()) & 1ull) T0 = t0;
            todo &= ~grp;
        }
        if (tri) {
            const int at   = n_tri + popc(m3 & lanes_below());
            io.tri_T0[at]  = T0;
            io.tri_T1[at]  = T_cur;
            io.tri_pc0[3 * at] = S.tri_tmp[k][0], io.tri_pc0[3 * at + 1] = S.tri_tmp[k][1], io.tri_pc0[3 * at + 2] = 1.0;
            io.tri_pc1[3 * at] = S.tri_tmp[k][2], io.tri_pc1[3 * at + 1] = S.tri_tmp[k][3], io.tri_pc1[3 * at + 2] = 1.0;
            S.tri_point_index[at] = k;
        }
        n_tri += popc(m3);
    }
    S.n_tri_index = n_tri;
    sync();
    *io.tri_count = n_tri;
    *io.tri_n_tcw = n_tcw;
    TC_MARK(35);
    return true;
}
TC_FN void finish_triangulation(Stream &S, const Cfg &C, const Io &io, const uint32_t *buckets_after, Scratch &X) {
    S.tri_queued     = 0;
    const Pose pose1 = S.frame[S.cur].pose;
    const int n      = S.n_tri_index;
    // pass 1 (parallel): the gates of :756-760 for every triangulated point -> accepted or not, its depth in the reference view, its
    // reference frame (scratch: X.next / X.key / X.bucket); either way the candidate leaves the list (:757 / :761)
    for (int q = lane(); q < n; q += NL) {
        const int k     = S.tri_point_index[q];
        const double *p = io.tri_pw + 3 * (S.tri_begin + q);
        const double pw[3]  = {p[0], p[1], p[2]};
        const int frame_ref = S.pts2d_ref_frame[k];
        const Pose pose0    = S.frame[frame_ref].pose;
        S.tri_status[k]     = 0;
        const bool good = is_good_to_track(C, S.tri_ref_undis[k], pose0, pw, 1.0, 3.0) && is_good_to_track(C, S.tri_cur_undis[k], pose1, pw, 1.0, 3.0);
        double pc[3];
        world2cam(pw, pose0, pc);
        X.next[q]   = good ? 1 : 0;
        X.key[q]    = double_as_key(pc[2]);
        X.bucket[q] = frame_ref;
    }
    sync();
    TC_MARK(41);
    // the frames that receive rows: the current one and the distinct reference frames of the accepted points, in order of first appearance
    int touched[10], touched_old[10], touched_cnt[10], n_touched = 0;
    touched[0] = S.cur, touched_old[0] = S.frame[S.cur].n_rows, touched_cnt[0] = 0, n_touched = 1;
    for (int q = 0; q < n; q++) {
        if (!X.next[q]) continue;
        const int fr = X.bucket[q];
        int tq = -1;
        for (int u = 0; u < n_touched; u++)
            if (touched[u] == fr) tq = u;
        if (tq < 0) {
            if (n_touched < 10) {
                touched[n_touched] = fr, touched_old[n_touched] = S.frame[fr].n_rows, touched_cnt[n_touched] = 0, n_touched++;
            } else {
                S.overflow |= OVF_TCW; // (more distinct reference frames than a window holds)
                X.next[q] = 0;
            }
        }
    }
    // pass 2 (parallel, a chunk of points per step): MapPoint::createMapPoint (mappoint.cc:25-49) and the two features (:769-784).  What the
    // one-by-one loop of the reference hands out in sequence is a function of the point's rank among the accepted ones: the r-th accepted
    // point takes the r-th map-point index the pool would pop (free list from the back, then fresh indices), id mappoint_id + r, row
    // n_rows + r of the current frame, and — ranked among the accepted points of ITS reference frame — the next row there
    const int n_free0 = S.n_free_mps, n_mps0 = S.n_mps, cur_rows0 = touched_old[0];
    const u64 id0     = S.mappoint_id;
    const u64 cur_fid = S.frame[S.cur].fid;
    const int unupd0  = S.frame[S.cur].n_unupd;
    int acc_before    = 0;
    for (int base = 0; base < n; base += NL) {
        const int q    = base + lane();
        const bool acc = q < n && X.next[q] != 0;
        const int fr   = acc ? X.bucket[q] : -1;
        const u64 m    = ballot(acc);
        const int r    = acc_before + popc(m & lanes_below());
        int tq = 0, rr = 0;
        for (int u = 1; u < n_touched; u++) { // (a triangulated point's reference frame is never the current frame: :723-730 re-anchors instead)
            const bool mine = acc && fr == touched[u];
            const u64 mu    = ballot(mine);
            if (mine) tq = u, rr = touched_cnt[u] + popc(mu & lanes_below());
            touched_cnt[u] += popc(mu);
        }
        if (acc) {
            const int k = S.tri_point_index[q];
            uint32_t i;
            if (r < n_free0) {
                i = S.free_mps[n_free0 - 1 - r];
            } else if (n_mps0 + (r - n_free0) < MAX_MPS) {
                i            = (uint32_t) (n_mps0 + (r - n_free0));
                S.hot[i].gen = 0;
            } else {
                S.overflow |= OVF_MPS;
                i = MAX_MPS - 1;
            }
            const int row_cur = cur_rows0 + r, row_ref = touched_old[tq] + rr;
            if (fr == S.cur || row_cur >= MAX_ROWS || row_ref >= MAX_ROWS || unupd0 + r >= MAX_ROWS) {
                S.overflow |= (fr == S.cur) ? OVF_INTERNAL : OVF_ROWS;
            } else {
                const double depth = key_as_double(X.key[q]);
                const double *p    = io.tri_pw + 3 * (S.tri_begin + q);
                MpHot h;
                memset(&h, 0, sizeof h);
                h.gen  = S.hot[i].gen;
                h.live = 1;
                h.type = (int8_t) MAPPOINT_TRIANGULATED;
                h.id   = id0 + (u64) r;
                h.pos[0] = p[0], h.pos[1] = p[1], h.pos[2] = p[2];
                h.observed = 2, h.used = 2; // addObservation + increaseUsedTimes for both features (:773-774, :780-781)
                h.last.frame = fr, h.last.gen = S.frame[fr].gen, h.last.row = row_ref;
                S.hot[i] = h;
                MpCold c;
                memset(&c, 0, sizeof c);
                c.born_fid  = cur_fid;
                c.ref_frame = fr;
                c.ref_gen   = S.frame[fr].gen;
                c.ref_kp    = S.tri_ref_undis[k];
                c.depth     = ((depth < 1.0) || (depth > 200.0)) ? 10.0 /*DEFAULT_DEPTH*/ : depth;
                S.cold[i]   = c;
                double pccx, pccy, pcrx, pcry;
                pixel2cam(C.cam, S.tri_cur_undis[k], pccx, pccy);
                pixel2cam(C.cam, S.tri_ref_undis[k], pcrx, pcry);
                Row a;
                a.id = h.id, a.mp = i, a.mpgen = h.gen, a.kp = S.tri_cur_undis[k], a.kpd = S.pts2d_cur[k];
                a.vel[0] = S.velocity_cur[k][0], a.vel[1] = S.velocity_cur[k][1], a.pcx = pccx, a.pcy = pccy;
                a.lk_idx = k < S.n_cand_lk ? S.cand_lk_idx[k] : -1, a.type = (int8_t) FEATURE_TRIANGULATED, a.outlier = 0, a.pad_[0] = a.pad_[1] = 0;
                S.frame[S.cur].row[row_cur] = a; // :769-774
                Row b;
                b.id = h.id, b.mp = i, b.mpgen = h.gen, b.kp = S.tri_ref_undis[k], b.kpd = S.pts2d_ref[k];
                b.vel[0] = S.velocity_ref[k][0], b.vel[1] = S.velocity_ref[k][1], b.pcx = pcrx, b.pcy = pcry;
                b.lk_idx = -1, b.type = (int8_t) FEATURE_TRIANGULATED, b.outlier = 0, b.pad_[0] = b.pad_[1] = 0;
                S.frame[fr].row[row_ref] = b; // :776-781 (a freshly drawn id is in no frame yet)
                S.frame[S.cur].unupd[unupd0 + r]     = i; // :784
                S.frame[S.cur].unupd_gen[unupd0 + r] = h.gen;
            }
        }
        acc_before += popc(m);
    }
    sync();
    TC_MARK(42);
    if (!S.overflow) {
        const int total = acc_before;
        const int from_free = total < n_free0 ? total : n_free0;
        S.n_free_mps = n_free0 - from_free;
        S.n_mps      = n_mps0 + (total - from_free);
        S.mappoint_id = id0 + (u64) total;
        S.frame[S.cur].n_rows  = cur_rows0 + total;
        S.frame[S.cur].n_unupd = unupd0 + total;
        for (int u = 1; u < n_touched; u++) S.frame[touched[u]].n_rows = touched_old[u] + touched_cnt[u];
    }
    sync();
    for (int u = 0; u < n_touched; u++) order_extend_auto(S.frame[touched[u]], touched_old[u], buckets_after, X);
    TC_MARK(43);
    const int nst = S.n_tri_status;
    const bool with_lk = S.n_cand_lk == nst;
    auto c_ref = compact(S.pts2d_ref, S.n_ref);
    auto c_rf = compact(S.pts2d_ref_frame, S.n_ref_frame);
    auto c_cur = compact(S.pts2d_cur, S.n_cur); // :788-793
    auto c_vr = compact2(S.velocity_ref, S.n_vel_ref);
    auto c_ru = compact(S.pts2d_ref_undis, S.n_ref_undis);
    auto c_cu = compact(S.tr_cur_undis, S.n_tr_cur_undis);

    auto c_lk = compact(S.cand_lk_idx, with_lk ? S.n_cand_lk : 0);
    reduce_vectors(S.tri_status, c_ref, c_rf, c_cur, c_vr, c_ru, c_cu, c_lk);
    S.n_ref = c_ref.kept, S.n_ref_frame = c_rf.kept, S.n_cur = c_cur.kept, S.n_vel_ref = c_vr.kept, S.n_ref_undis = c_ru.kept, S.n_tr_cur_undis = c_cu.kept;
    if (with_lk) S.n_cand_lk = c_lk.kept;
    TC_MARK(44);
    copy_n(S.pts2d_new, S.pts2d_cur, S.n_cur);
    S.n_new = S.n_cur;
    copy_n(S.pts2d_new_undis, S.tr_cur_undis, S.n_tr_cur_undis);
    S.n_new_undis = S.n_tr_cur_undis;
}

TC_FN void make_new_frame_queue(Stream &S, const Cfg &C, Io &io, int state, Scratch &X) { // :251-261
    set_keyframe(S, S.cur, state);
    S.isnewkeyframe = 1;
    if ((state == KEYFRAME_NORMAL) || (state == KEYFRAME_REMOVE_OLDEST)) {
        S.ref = S.cur;
        queue_detection(S, C, io, S.ref, true, X);
    }
}

// ---- the stages (TableTracker::beginFrame / advance; the device primitive that runs after each stage is named) --------------------------
// stage 0 -> preprocess
TC_FN void stage_begin_frame(Stream &S, Io &io, double stamp, const Pose &pose, u64 image) {
    S.done          = 0;
    S.result        = TRACK_PASSED;
    S.isnewkeyframe = 0; // :108
    S.log_valid     = 0;
    S.mode          = M_NONE;
    S.det_job       = -1;
    S.rs_set        = -1;
    S.tri_queued    = 0;
    S.lk_map_n = S.lk_ref_n = 0;
    S.ref_tracked   = 0;
    S.pending       = frame_alloc(S);
    Frame &f        = S.frame[S.pending];
    f.fid           = S.frame_id++; // frame.cc:37-40
    S.last_input_fid = f.fid;
    f.stamp         = stamp;
    f.pose          = pose;
    f.image         = image;
    S.pending_slot  = slot_alloc(S);
    *io.pre_slot    = S.pending_slot;
    // nothing else is queued yet
    *io.det_slot       = -1;
    *io.det_mask_count = 0;
    *io.lk_count       = 0;
    *io.rs_count       = 0;
    *io.tri_count      = 0;
    *io.tri_n_tcw      = 0;
}
// stage 1 (after preprocess) -> detection A
TC_FN void stage_on_preprocess(Stream &S, const Cfg &C, Io &io, Scratch &X) {
    if (S.done) return;
    if (C.check_histogram) { // :115-133
        const double hist = *io.pre_hist;
        if (S.histogram != 0) {
            const double rate = tc_fabs((hist - S.histogram) / S.histogram);
            if (rate > 0.1) {
                S.passed_cnt++;
                if (S.passed_cnt > 1) S.histogram = 0;
                slot_free(S, S.pending_slot);
                S.pending_slot = -1;
                frame_free(S, S.pending);
                S.pending = -1;
                finish(S, TRACK_PASSED);
                return;
            }
        }
        S.histogram = hist;
    }
    S.det_job = -1;
    S.pre     = S.cur; // :135
    S.cur     = S.pending;
    S.pending = -1;
    assign_slot(S, S.cur);
    release_unused_slots(S);
    if (S.isinitializing) {
        if (S.ref < 0) { // :158-166
            do_reset_tracking(S);
            S.ref  = S.cur;
            S.mode = M_FIRST;
            queue_detection(S, C, io, S.ref, false, X);
            return;
        }
        S.mode = M_INIT;
        if (S.n_ref == 0) queue_detection(S, C, io, S.ref, false, X); // :168-170
    } else {
        S.mode = M_TRACK;
    }
}
// stage 2 (after detection A) -> LK
TC_FN void stage_on_detect_a(Stream &S, const Cfg &C, Io &io, Scratch &X) {
    if (S.done) return;
    if (S.det_job >= 0) integrate_detection(S, C, io);
    *io.det_slot = -1;
    if (S.mode == M_FIRST) {
        release_unused_slots(S);
        finish(S, TRACK_FIRST_FRAME);
        return;
    }
    *io.lk_count = 0;
    if (S.mode == M_TRACK) queue_track_mappoint(S, C, io, X); // :206
    queue_track_reference(S, C, io);                        // :173 / :209
}
// stage 3 (after LK) -> RANSAC
TC_FN void stage_on_lk(Stream &S, const Cfg &C, Io &io, const uint32_t *buckets_after, Scratch &X) {
    if (S.done) return;
    if (S.mode == M_TRACK) finish_track_mappoint(S, C, io, buckets_after, X);
    S.ref_tracked = mid_track_reference(S, C, io, X) ? 1 : 0;
    TC_MARK(25);
    *io.lk_count  = 0;
}
// stage 4 (after RANSAC) -> triangulation
TC_FN void stage_on_ransac(Stream &S, const Cfg &C, Io &io, Scratch &X) {
    if (S.done) return;
    if (S.ref_tracked) finish_track_reference(S, io);
    TC_MARK(30);
    *io.rs_count = 0;
    if (S.mode == M_INIT) {
        if (S.parallax_ref < C.track_min_parallax) { // :175-178
            finish(S, TRACK_INITIALIZING);
            return;
        }
        queue_triangulation(S, C, io, X); // :182
        return;
    }
    S.kf_state = check_keyframe_state(S, C); // :212
    TC_MARK(31);
    if ((S.kf_state == KEYFRAME_NORMAL) || (S.kf_state == KEYFRAME_REMOVE_OLDEST)) queue_triangulation(S, C, io, X); // :215-217
}
// stage 5 (after triangulation) -> detection B
TC_FN void stage_on_triangulate(Stream &S, const Cfg &C, Io &io, const uint32_t *buckets_after, Scratch &X) {
    if (S.done) return;
    if (S.tri_queued) finish_triangulation(S, C, io, buckets_after, X);
    TC_MARK(45);
    *io.tri_count = 0;
    if (S.mode == M_INIT) {
        if (do_reset_tracking(S)) { // :184-190
            S.lost_reset = 1;
            make_new_frame_queue(S, C, io, KEYFRAME_NORMAL, X);
            return;
        }
        S.lost_reset = 0;
        set_keyframe(S, S.ref, KEYFRAME_NORMAL);         // :193
        make_new_frame_queue(S, C, io, KEYFRAME_NORMAL, X); // :196
        S.last_keyframe  = S.cur;
        S.isinitializing = 0;
        return;
    }
    S.lost_reset = 0;
    if (!S.frame[S.cur].n_rows) { // :224
        do_reset_tracking(S);
        S.lost_reset = 2;
        make_new_frame_queue(S, C, io, KEYFRAME_NORMAL, X); // :225
        return;
    }
    if ((S.kf_state == KEYFRAME_NORMAL) || (S.kf_state == KEYFRAME_REMOVE_OLDEST)) {
        make_new_frame_queue(S, C, io, S.kf_state, X); // :230-232
    } else {
        queue_detection(S, C, io, S.cur, true, X); // :220
        if (S.kf_state != KEYFRAME_NONE) make_new_frame_queue(S, C, io, S.kf_state, X); // REMOVE_SECOND_NEW: flags only
    }
}
// stage 6 (after detection B): the frame is done
TC_FN void stage_on_detect_b(Stream &S, const Cfg &C, Io &io) {
    if (S.done) return;
    if (S.det_job >= 0) integrate_detection(S, C, io);
    *io.det_slot = -1;
    release_unused_slots(S);
    if (S.mode == M_INIT) {
        finish(S, S.lost_reset == 1 ? TRACK_FIRST_FRAME : TRACK_TRACKING);
        return;
    }
    if (S.lost_reset == 2) {
        finish(S, TRACK_LOST);
        return;
    }
    finish(S, TRACK_TRACKING);
}

// ---- after the frame: statistics, digest, sliding-window stand-in (TrackingBatch::step, TableTracker::endFrame) ---------------------------
TC_FN void fnv(u64 &h, const void *p, int n) {
    const unsigned char *c = (const unsigned char *) p;
    for (int i = 0; i < n; i++) {
        h ^= c[i];
        h *= 1099511628211ull;
    }
}
TC_FN u64 mix64(u64 x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
TC_FN void stage_end_frame(Stream &S, const Cfg &C) {
    const int st = S.result;
    S.last_state = st;
    S.frames++;
    if (S.isnewkeyframe || st == TRACK_FIRST_FRAME || st == TRACK_LOST) S.keyframes++;
    {
        int32_t sti = st;
        fnv(S.digest, &sti, sizeof sti);
        u64 fid = S.last_input_fid;
        fnv(S.digest, &fid, sizeof fid);
        if (st != TRACK_PASSED) {
            u64 acc = 0, cnt = 0;
            if (S.cur >= 0) { // order-independent combination of per-feature hashes: a partial sum per lane
                const Frame &fr = S.frame[S.cur];
                for (int q = lane(); q < fr.n_rows; q += NL) {
                    u64 bits;
                    memcpy(&bits, &fr.row[q].kpd, sizeof bits);
                    acc += mix64(mix64(fr.row[q].id) ^ bits);
                }
                acc = wave_sum(acc);
                cnt = (u64) fr.n_rows;
            }
            fnv(S.digest, &acc, sizeof acc);
            fnv(S.digest, &cnt, sizeof cnt);
            S.tracked_sum += cnt;
            u64 nref = (u64) S.n_new;
            fnv(S.digest, &nref, sizeof nref);
        }
    }
    TC_MARK(52);
    // WindowKeeper::onFrame (ic_gvins.cc:542, 743, 1391-1410, 445-448, 1675)
    const int frame = S.cur;
    if (st != TRACK_PASSED && frame >= 0 && (S.isnewkeyframe || st == TRACK_FIRST_FRAME || st == TRACK_LOST)) {
        map_insert_keyframe(S, C, frame);
        TC_MARK(53);
        // (ic_gvins.cc:1391-1410 walks the keyframes in id order and drops those flagged REMOVE_SECOND_NEW and the empty ones except the newest;
        // a decision reads its own frame and the newest id only, and erasing an entry keeps the order of the others: the walk's order is
        // immaterial — an entry per lane)
        {
            const int n = S.n_map_kf;
            u64 newest  = 0;
            for (int base = 0; base < n; base += NL) {
                const int k = base + lane();
                const u64 v = wave_max(k < n ? S.map_kf_key[k] : 0);
                newest      = v > newest ? v : newest;
            }
            int kept = 0;
            for (int base = 0; base < n; base += NL) {
                const int k = base + lane();
                bool keep = false, drop = false;
                u64 id    = 0;
                int h     = 0;
                if (k < n) {
                    id       = S.map_kf_key[k];
                    h        = S.map_kf_frame[k];
                    Frame &f = S.frame[h];
                    drop     = (f.kf_state == KEYFRAME_REMOVE_SECOND_NEW) || ((f.n_rows == 0) && (id != newest));
                    keep     = !drop;
                    if (drop) {
                        f.is_kf    = 0; // resetKeyFrame (frame.h:58-63); the keyframe id stays
                        f.kf_state = KEYFRAME_NONE;
                    }
                }
                const u64 m = ballot(keep);
                sync(); // (the chunk is read before its entries move down: map_remove_keyframe(S, h, false) for each dropped one)
                if (keep) S.map_kf_key[kept + popc(m & lanes_below())] = id, S.map_kf_frame[kept + popc(m & lanes_below())] = h;
                kept += popc(m);
                sync();
            }
            S.n_map_kf = kept;
        }
        while (S.n_map_kf > C.window_size) {
            const int n = S.n_map_kf;
            u64 oldest  = ~0ull;
            for (int base = 0; base < n; base += NL) {
                const int k = base + lane();
                const u64 v = wave_min(k < n ? S.map_kf_key[k] : ~0ull);
                oldest      = v < oldest ? v : oldest;
            }
            const int at = map_find_wave(S, oldest); // (keys are distinct; the one-by-one scan keeps the first minimum, the only one)
            map_remove_keyframe(S, S.map_kf_frame[at], true);
        }
        TC_MARK(54);
    }
    sweep_frames(S);
    TC_MARK(55);
}

// ---- a fresh stream --------------------------------------------------------------------------------------------------------------------
TC_FN void stream_init(Stream &S, int first_slot) {
    // (the caller zero-fills the block first: memset / hipMemset)
    S.cur = S.ref = S.pre = S.last_keyframe = S.pending = S.latest_keyframe = S.det_frame = -1;
    S.isinitializing = 1;
    S.done           = 1;
    S.result         = TRACK_PASSED;
    S.pending_slot   = -1;
    S.det_job        = -1;
    S.rs_set         = -1;
    S.kf_state       = KEYFRAME_NONE;
    S.last_state     = TRACK_PASSED;
    S.digest         = 1469598103934665603ull;
    S.n_free_slots   = MAX_SLOTS;
    for (int k = 0; k < MAX_SLOTS; k++) S.free_slots[k] = first_slot + MAX_SLOTS - 1 - k; // popped in ascending order
}

} // namespace tc
