// C entry points of libicgvins_host.so for harnesses that cannot speak C++ (tests, bench.py): drive a TrackingBatch, its maps and windows.
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>
#include <atomic>
#include <mutex>

#include "tracking_batch.h"
#include "hostprof.h"

#include "solver_hip.h"
#include "solver_batch_hip.h"
#include "culling_hip.h"
#include "window_visual.h"
#include "capi_windows.h"

using namespace icg;

struct icgh_batch {
    std::unique_ptr<StreamGroups> tb;
    int w, h;
    bool cams_differ{false}; // icgh_batch_create_cams with cameras that are not all bit-equal
};

namespace {
TrackingConfig batch_config(int max_features, double min_parallax, double max_interval, int check_hist, double reproj_std) {
    TrackingConfig cfg;
    cfg.track_max_features     = max_features;
    cfg.track_min_parallax     = min_parallax;
    cfg.track_max_interval     = max_interval;
    cfg.track_check_histogram  = check_hist != 0;
    cfg.reprojection_error_std = reproj_std;
    return cfg;
}

// A culling entry of the batch's stream s: its map, its list, and — in a batch with per-stream cameras — its camera and the index of that
// camera in its group's table (the stream's local index; -1 where the group's cameras are all equal and the group keeps a single camera)
WindowCulling::Stream culling_stream(icgh_batch *b, int s, const std::unordered_map<ulong, double> *list) {
    WindowCulling::Stream S{b->tb->stream(s).objectMap(), list};
    if (b->cams_differ) {
        S.camera    = b->tb->stream(s).camera;
        S.cam_index = b->tb->group(b->tb->groupOf(s)).device()->cameraTableSize() > 0 ? b->tb->localOf(s) : -1;
    }
    return S;
}

// One WindowCulling call for all streams on group 0's context, as ever, where the batch has one camera.  With per-stream cameras a
// group's table lives on the group's own context and is indexed by the local stream: one call per group, on its context.
// stream_of[k]: the batch's stream of streams[k].
template <typename R, typename Fn>
bool cull_by_context(icgh_batch *b, const vector<WindowCulling::Stream> &streams, const vector<int> &stream_of, vector<R> &out, std::string *e, Fn &&call) {
    if (!b->cams_differ) return call(b->tb->group(0).device()->ctx(), streams, out, e);
    out.assign(streams.size(), R());
    for (int g = 0; g < b->tb->groups(); g++) {
        vector<WindowCulling::Stream> part;
        vector<size_t> at;
        for (size_t k = 0; k < streams.size(); k++)
            if (b->tb->groupOf(stream_of[k]) == g) part.push_back(streams[k]), at.push_back(k);
        if (part.empty()) continue;
        vector<R> r;
        if (!call(b->tb->group(g).device()->ctx(), part, r, e)) return false;
        for (size_t j = 0; j < at.size(); j++) out[at[j]] = r[j];
    }
    return true;
}
} // namespace


extern "C" {

icgh_batch *icgh_batch_create(int device, int n_streams, const double *cam10, int w, int h, int max_features,
                              double min_parallax, double max_interval, int check_hist, double reproj_std, int window,
                              int host_threads, int n_groups, char *err, int errlen) {
    return guarded(err, errlen, (icgh_batch *) nullptr, [&] {
        const TrackingConfig cfg = batch_config(max_features, min_parallax, max_interval, check_hist, reproj_std);
        vector<double> intr{cam10[0], cam10[1], cam10[2], cam10[3], cam10[4]};
        vector<double> dist{cam10[5], cam10[6], cam10[7], cam10[8], cam10[9]};
        std::unique_ptr<icgh_batch> b(new icgh_batch());
        b->w = w;
        b->h = h;
        b->tb.reset(new StreamGroups(device, n_streams, n_groups, intr, dist, {w, h}, cfg, window, host_threads));
        return b.release();
    });
}

// icgh_batch_create with a calibration per stream: cams = n_streams x 10 doubles (fx, fy, cx, cy, skew, k1, k2, p1, p2, k3 per stream).
// Fails (NULL, the reason in err) where the cameras differ and the C ABI underneath has no camera-table entries.
icgh_batch *icgh_batch_create_cams(int device, int n_streams, const double *cams, int w, int h, int max_features, double min_parallax,
                                   double max_interval, int check_hist, double reproj_std, int window, int host_threads, int n_groups, char *err,
                                   int errlen) {
    return guarded(err, errlen, (icgh_batch *) nullptr, [&] {
        if (!cams || n_streams <= 0) throw std::runtime_error("icgh_batch_create_cams: no cameras");
        const TrackingConfig cfg = batch_config(max_features, min_parallax, max_interval, check_hist, reproj_std);
        vector<vector<double>> intr, dist;
        for (int i = 0; i < n_streams; i++) {
            const double *c = cams + 10 * (size_t) i;
            intr.emplace_back(c, c + 5);
            dist.emplace_back(c + 5, c + 10);
        }
        std::unique_ptr<icgh_batch> b(new icgh_batch());
        b->w = w;
        b->h = h;
        b->cams_differ = false;
        for (int i = 1; i < n_streams; i++) b->cams_differ |= memcmp(cams, cams + 10 * (size_t) i, 10 * sizeof(double)) != 0;
        b->tb.reset(new StreamGroups(device, n_streams, n_groups, intr, dist, {w, h}, cfg, window, host_threads));
        return b.release();
    });
}

void icgh_batch_destroy(icgh_batch *b) { delete b; }

int icgh_batch_groups(icgh_batch *b) { return b ? b->tb->groups() : 0; }
void *icgh_batch_ctx(icgh_batch *b, int group) {
    return (b && group >= 0 && group < b->tb->groups()) ? (void *) b->tb->group(group).device()->ctx() : nullptr;
}

// K lock-step frames for every stream in one call (K = 1: the classic per-frame step).
// images[k*n + i]: pointer to the frame of stream i at step k (host or device memory), NULL to idle the stream that step.
// stamps[k*n + i]; poses12[(k*n + i)*12 ..] = R (camera->world, row-major) | t, the INS prior the reference sets with
// frame->setPose().  states[k*n + i] receives the TrackState.  Groups do not wait for each other between the K steps.
int icgh_batch_run(icgh_batch *b, int K, const void *const *images, int stride, int channels, int on_device,
                   const double *stamps, const double *poses12, int32_t *states, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const int n = b->tb->size();
        auto t0     = std::chrono::steady_clock::now();
        vector<vector<FrameInput>> frames((size_t) K, vector<FrameInput>((size_t) n));
        for (int k = 0; k < K; k++)
            for (int i = 0; i < n; i++) {
                const size_t j = (size_t) k * n + i;
                if (!images[j]) continue;
                FrameInput &f = frames[(size_t) k][(size_t) i];
                f.valid       = true;
                f.stamp       = stamps[j];
                f.image       = Mat::wrap((uint8_t *) images[j], b->h, b->w, channels, (size_t) stride, on_device != 0);
                f.pose        = poseFromArray12(poses12 + 12 * j);
            }
        vector<vector<TrackState>> st;
        auto t1 = std::chrono::steady_clock::now();
        b->tb->stepMany(frames, st);
        auto t2 = std::chrono::steady_clock::now();
        for (int k = 0; k < K; k++)
            for (int i = 0; i < n; i++) states[(size_t) k * n + i] = (int32_t) st[(size_t) k][(size_t) i];
        frames.clear();
        auto t3 = std::chrono::steady_clock::now();
        if (getenv("ICG_DEBUG_TIMING"))
            fprintf(stderr, "[icgh_batch_run] K=%d create %.2f ms, stepMany %.2f ms, teardown %.2f ms\n", K,
                    std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count(),
                    std::chrono::duration<double, std::milli>(t3 - t2).count());
        return 0;
    });
}

int icgh_batch_step(icgh_batch *b, const void *const *images, int stride, int channels, int on_device, const double *stamps,
                    const double *poses12, int32_t *states, char *err, int errlen) {
    return icgh_batch_run(b, 1, images, stride, channels, on_device, stamps, poses12, states, err, errlen);
}

// out: frames, keyframes, tracked_sum, digest, mappoints created, keyframes in window, landmarks in map, last state
int icgh_batch_stats(icgh_batch *b, int stream, uint64_t *out8) {
    if (!b || stream < 0 || stream >= b->tb->size()) return -1;
    auto &s = b->tb->stream(stream);
    out8[0] = s.frames;
    out8[1] = s.keyframes;
    out8[2] = s.tracked_sum;
    out8[3] = s.digest;
    out8[4] = s.ids->mappoint_id;
    out8[5] = s.windowKeyFrames();
    out8[6] = s.landmarks();
    out8[7] = (uint64_t) s.last_state;
    return 0;
}

// the same for every stream in one call (n x 8): the bench reads the statistics of hundreds of streams between its warm-up and its timed
// region, where every millisecond the GPU idles costs clock state
int icgh_batch_stats_all(icgh_batch *b, uint64_t *out8n) {
    if (!b || !out8n) return -1;
    for (int i = 0; i < b->tb->size(); i++)
        if (icgh_batch_stats(b, i, out8n + 8 * (size_t) i) != 0) return -1;
    return 0;
}

int icgh_batch_timing(icgh_batch *b, double *out5, int reset) {
    if (!b) return -1;
    for (int i = 0; i < 5; i++) out5[i] = 0;
    for (int g = 0; g < b->tb->groups(); g++)
        for (int i = 0; i < 5; i++) {
            out5[i] += b->tb->group(g).timing[i] / b->tb->groups(); // mean over groups (they run concurrently)
            if (reset) b->tb->group(g).timing[i] = 0;
        }
    return 0;
}

// work counters summed over the groups (see TrackingBatch::counters); reset != 0 clears them
int icgh_batch_counters(icgh_batch *b, uint64_t *out8, int reset) {
    if (!b) return -1;
    for (int i = 0; i < 8; i++) out8[i] = 0;
    for (int g = 0; g < b->tb->groups(); g++)
        for (int i = 0; i < 8; i++) {
            out8[i] += b->tb->group(g).counters[i];
            if (reset) b->tb->group(g).counters[i] = 0;
        }
    return 0;
}

// per-step log of group g since the last reset: out[3k..3k+2] = {steady-clock seconds at the end of the step, host-logic
// seconds, device-execute seconds}; returns the number of steps written (<= max_steps); reset != 0 clears the log
int icgh_batch_step_log(icgh_batch *b, int g, double *out, int max_steps, int reset) {
    if (!b || g < 0 || g >= b->tb->groups()) return -1;
    auto &log = b->tb->group(g).step_log;
    int n     = (int) std::min<size_t>(log.size(), (size_t) std::max(0, max_steps));
    for (int k = 0; k < n && out; k++) {
        out[3 * k]     = log[(size_t) k].t_end;
        out[3 * k + 1] = log[(size_t) k].host_logic;
        out[3 * k + 2] = log[(size_t) k].device_execute;
    }
    if (reset) log.clear();
    return n;
}

// steady-clock seconds on the clock icgh_batch_step_log reports
double icgh_now_s(void) { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int icgh_batch_timing_group(icgh_batch *b, int g, double *out5) {
    if (!b || g < 0 || g >= b->tb->groups()) return -1;
    for (int i = 0; i < 5; i++) out5[i] = b->tb->group(g).timing[i];
    return 0;
}

// section timers of the host layer (ICG_HOST_PROF=1): out[2k] = seconds, out[2k+1] = calls; names are ';'-separated
int icgh_hostprof(double *out, int max_sections, char *names, int names_len, int reset) {
    int n = std::min(max_sections, (int) icg::hostprof::N_SECTIONS);
    std::string nm;
    for (int k = 0; k < n; k++) {
        out[2 * k]     = 1e-9 * (double) icg::hostprof::ns()[k].load();
        out[2 * k + 1] = (double) icg::hostprof::calls()[k].load();
        nm += icg::hostprof::name(k);
        nm += ';';
        if (reset) {
            icg::hostprof::ns()[k]    = 0;
            icg::hostprof::calls()[k] = 0;
        }
    }
    if (names && names_len > 0) snprintf(names, (size_t) names_len, "%s", nm.c_str());
    return n;
}

// the tracker's un-triangulated candidate points in list order: cur[2k..] (pts2d_new_), ref[2k..] (pts2d_ref_)
int icgh_batch_candidates(icgh_batch *b, int stream, int max, float *cur, float *ref) {
    if (!b || stream < 0 || stream >= b->tb->size()) return -1;
    const auto &pn = b->tb->stream(stream).trackedRefPoints();
    const auto &pr = b->tb->stream(stream).referencePoints();
    int n = (int) std::min(pn.size(), pr.size());
    if (n > max) n = max;
    for (int k = 0; k < n; k++) {
        cur[2 * k] = pn[(size_t) k].x, cur[2 * k + 1] = pn[(size_t) k].y;
        ref[2 * k] = pr[(size_t) k].x, ref[2 * k + 1] = pr[(size_t) k].y;
    }
    return (pn.size() == pr.size()) ? n : -2;
}

// features of the stream's current frame, sorted by map-point id: ids[k], px[2k..2k+1] (distorted keypoint)
int icgh_batch_features(icgh_batch *b, int stream, int max, uint64_t *ids, float *px) {
    if (!b || stream < 0 || stream >= b->tb->size()) return -1;
    vector<std::pair<ulong, Point2f>> v;
    b->tb->stream(stream).currentFeatures(v);
    std::sort(v.begin(), v.end(), [](const auto &a, const auto &c) { return a.first < c.first; });
    int n = 0;
    for (const auto &kv : v) {
        if (n >= max) break;
        ids[n]        = kv.first;
        px[2 * n]     = kv.second.x;
        px[2 * n + 1] = kv.second.y;
        n++;
    }
    return n;
}

// Kernel-only ceiling: icgh_batch_record(b, 1); <one icgh_batch_run step>; icgh_batch_record(b, 0); then icgh_batch_replay(b, reps) issues the
// recorded device calls of every group again — one group after the other, nothing else on the GPU, no tracker logic — so that the HIP-event
// times of icg_prof_* are the EXCLUSIVE device times of the step's kernels.  Returns the number of recorded stage batches (all groups).
int icgh_batch_record(icgh_batch *b, int on) {
    if (!b) return -1;
    for (int g = 0; g < b->tb->groups(); g++) b->tb->group(g).record(on != 0);
    return 0;
}
int icgh_batch_replay(icgh_batch *b, int reps, char *err, int errlen) {
    if (!b) return -1;
    return guarded(err, errlen, -2, [&] {
        int n = 0;
        for (int g = 0; g < b->tb->groups(); g++) {
            b->tb->group(g).replay(reps);
            n += (int) b->tb->group(g).device()->recorded();
        }
        return n;
    });
}

// the same recorded calls issued by ALL groups at once from their own threads (the concurrency of a real run, no tracker logic)
int icgh_batch_replay_concurrent(icgh_batch *b, int reps, char *err, int errlen) {
    if (!b) return -1;
    return guarded(err, errlen, -2, [&] {
        b->tb->replayAll(reps);
        return 0;
    });
}

// 0 = track table (default), 1 = object graph (ICG_TRACK_ENGINE=object)
int icgh_batch_engine(icgh_batch *b) { return b ? (int) b->tb->group(0).engine() : -1; }

// canonical text dump of a stream's tracker + map state (engine-vs-engine tests): kind 0 = the engine's state, 1 = the map part of the
// table engine's state, 2 = the same text computed from the table engine's materialized object graph (B2 view).  Returns the length
// of the text (the buffer receives at most len-1 characters), -1 on bad arguments.
long icgh_batch_dump(icgh_batch *b, int stream, int kind, char *out, long len) {
    if (!b || stream < 0 || stream >= b->tb->size()) return -1;
    return guarded(nullptr, 0, -2L, [&] {
        const std::string s = b->tb->stream(stream).dump(kind);
        if (out && len > 0) {
            const size_t n = std::min((size_t) len - 1, s.size());
            memcpy(out, s.data(), n);
            out[n] = 0;
        }
        return (long) s.size();
    });
}

// ---- f3: outlier culling / statistics (culling_hip.h) on the maps the tracker built -------------------------------------------
// Raw dump of a stream's landmark graph, NO filtering (the test re-derives the reference's filters and decisions from it):
// landmarks sorted by id: lm_id, lm_pos[3], lm_flags (bit0 outlier), lm_ref_frame (frame id), lm_obs_off[n+1];
// observations in list order: obs_frame (frame id, ~0 = expired), obs_flags (bit0 feature expired, bit1 feature outlier,
// bit2 frame is keyframe, bit3 keyframe in map), obs_pose12, obs_pix[2] (undistorted key point).  Returns the landmark count.
int icgh_batch_landmark_table(icgh_batch *b, int stream, int max_lm, int max_obs, uint64_t *lm_id, double *lm_pos, int32_t *lm_flags,
                              uint64_t *lm_ref_frame, int32_t *lm_obs_off, uint64_t *obs_frame, int32_t *obs_flags, double *obs_pose12,
                              float *obs_pix) {
    if (!b || stream < 0 || stream >= b->tb->size()) return -1;
    auto &S       = b->tb->stream(stream);
    Map::Ptr Smap = S.objectMap(); // (track-table engine: a view of the table as reference-shaped objects; read-only use here)
    vector<ulong> ids;
    for (auto &kv : Smap->landmarks()) ids.push_back(kv.first);
    std::sort(ids.begin(), ids.end());
    if ((int) ids.size() > max_lm) return -2;
    int no = 0;
    for (size_t k = 0; k < ids.size(); k++) {
        auto mp      = Smap->landmarks().at(ids[k]);
        lm_id[k]     = ids[k];
        Vector3d pos = mp->pos();
        for (int c = 0; c < 3; c++) lm_pos[3 * k + c] = pos[c];
        lm_flags[k]     = mp->isOutlier() ? 1 : 0;
        lm_ref_frame[k] = mp->referenceFrameId();
        lm_obs_off[k]   = no;
        for (auto &w : mp->observations()) {
            if (no >= max_obs) return -3;
            auto feat = w.lock();
            int fl    = 0;
            obs_frame[no] = ~0ull;
            for (int c = 0; c < 12; c++) obs_pose12[12 * (size_t) no + c] = 0;
            obs_pix[2 * no] = obs_pix[2 * no + 1] = 0;
            if (!feat) {
                fl |= 1;
            } else {
                if (feat->isOutlier()) fl |= 2;
                obs_pix[2 * no] = feat->keyPoint().x, obs_pix[2 * no + 1] = feat->keyPoint().y;
                auto frame = feat->getFrame();
                if (frame) {
                    obs_frame[no] = frame->id();
                    if (frame->isKeyFrame()) fl |= 4;
                    if (frame->isKeyFrame() && Smap->isKeyFrameInMap(frame)) fl |= 8;
                    Pose p = frame->pose();
                    poseToArray12(p, obs_pose12 + 12 * (size_t) no);
                }
            }
            obs_flags[no] = fl;
            no++;
        }
    }
    lm_obs_off[ids.size()] = no;
    return (int) ids.size();
}

// moves landmarks (by id) to new positions: stands in for the optimizer's write-back (ic_gvins.cc:1299-1357) in the tests
int icgh_batch_set_landmark_pos(icgh_batch *b, int stream, int n, const uint64_t *ids, const double *pos3) {
    if (!b || stream < 0 || stream >= b->tb->size()) return -1;
    auto &S       = b->tb->stream(stream);
    Map::Ptr Smap = S.objectMap();
    int rc        = 0;
    for (int k = 0; k < n && rc == 0; k++) {
        auto it = Smap->landmarks().find(ids[k]);
        if (it == Smap->landmarks().end())
            rc = -2;
        else
            it->second->setPos(Vector3d(pos3[3 * k], pos3[3 * k + 1], pos3[3 * k + 2]));
    }
    S.commitMap(); // (track-table engine: the new positions go into the table)
    return rc;
}

namespace {
// Views of the streams' maps (TrackingBatch::Stream::objectMap) that an entry point mutates: committed to the track tables only when the
// entry point ran to its end (commit()); on an exception or an early error return every view is dropped unabsorbed, so the tables keep the
// state they had and no later objectMap() sees a half-modified view.
struct MapViewsGuard {
    explicit MapViewsGuard(icgh_batch *batch) : b(batch) {}
    ~MapViewsGuard() {
        if (done) return;
        for (int s = 0; s < b->tb->size(); s++) b->tb->stream(s).discardMap();
    }
    void commit() {
        for (int s = 0; s < b->tb->size(); s++) b->tb->stream(s).commitMap();
        done = true;
    }
    icgh_batch *b;
    bool done{false};
};
} // namespace

// WindowCulling over ALL streams of the batch with one device launch.  in_list: per stream the landmark ids that "took part in
// the optimization" (invdepthlist_), concatenated, list_off[n_streams+1].  mode 0: gvinsOutlierCulling -> out5[s*5..] =
// outlier mappoints, outlier features, num1, num2, num3;  mode 1: reprojectionStatistics -> stats5[s*5..] = min, max, avg, rms, count
int icgh_batch_culling(icgh_batch *b, int mode, const int32_t *list_off, const uint64_t *in_list, double reprojection_error_std, int32_t *out5,
                       double *stats5, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const int n = b->tb->size();
        MapViewsGuard views(b);
        vector<std::unordered_map<ulong, double>> lists((size_t) n);
        vector<WindowCulling::Stream> streams;
        for (int s = 0; s < n; s++) {
            for (int k = list_off[s]; k < list_off[s + 1]; k++) lists[(size_t) s][in_list[k]] = 0.0;
            streams.push_back(culling_stream(b, s, &lists[(size_t) s]));
        }
        vector<int> stream_of((size_t) n);
        for (int s = 0; s < n; s++) stream_of[(size_t) s] = s;
        std::string e;
        if (mode == 0) {
            vector<CullingResult> R;
            if (!cull_by_context(b, streams, stream_of, R, &e, [&](icg_ctx *ctx, const vector<WindowCulling::Stream> &part, vector<CullingResult> &r, std::string *pe) {
                    return WindowCulling::gvinsOutlierCulling(ctx, part, reprojection_error_std, r, pe);
                })) {
                set_err(err, errlen, e.c_str());
                return -2;
            }
            for (int s = 0; s < n; s++) {
                const CullingResult &r = R[(size_t) s];
                const int32_t v[5]     = {r.outlier_mappoints, r.outlier_features, r.by_reference_frame, r.by_observation_count, r.by_mean_error};
                memcpy(out5 + 5 * s, v, sizeof v);
            }
        } else {
            vector<ReprojectionStatistics> R;
            if (!cull_by_context(b, streams, stream_of, R, &e, [&](icg_ctx *ctx, const vector<WindowCulling::Stream> &part, vector<ReprojectionStatistics> &r, std::string *pe) {
                    return WindowCulling::reprojectionStatistics(ctx, part, r, pe);
                })) {
                set_err(err, errlen, e.c_str());
                return -2;
            }
            for (int s = 0; s < n; s++) {
                const ReprojectionStatistics &r = R[(size_t) s];
                const double v[5]               = {r.min_error, r.max_error, r.avg_error, r.rms_error, (double) r.landmarks};
                memcpy(stats5 + 5 * s, v, sizeof v);
            }
        }
        views.commit(); // (track-table engine: flags, counters and removals go into the table)
        return 0;
    });
}

// ---- map -> optimizer -> map on the windows the tracker built (window_visual.h + solver_hip.h + culling_hip.h) ----------------
// For every stream: VisualWindow::build (addReprojectionParameters / addReprojectionFactors), pose priors at the current keyframe
// poses (weight prior_weight; they stand in for the IMU / GNSS / marginalization factors), LM solve - chi-square culling - LM solve,
// updateParametersFromOptimizer, gvinsOutlierCulling.  out7[s*7..] = keyframes, factors, initial cost, final cost, removed by chi2,
// culled map points, culled features.  kf_out (optional, max_kf rows of 14 per stream): keyframe stamp, frame id, camera pose12.
int icgh_batch_refine_windows(icgh_batch *b, const double *pose_b_c12, double td, double reprojection_error_std, double prior_weight, int iters1,
                              int iters2, double chi2, double *out7, int max_kf, double *kf_out, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const int n = b->tb->size();
        MapViewsGuard views(b);
        Pose pbc;
        pbc = poseFromArray12(pose_b_c12);
        const bool lockstep = getenv("ICG_REFINE_PER_STREAM") == nullptr; // default: all streams' windows in ONE WindowSolverBatch
        vector<std::unique_ptr<VisualWindow>> wins;
        vector<vector<vector<double>>> priors((size_t) n);
        vector<int> slot((size_t) n, -1);
        WindowSolverBatch batch(0, 1.0);
        for (int s = 0; s < n; s++) {
            auto &S = b->tb->stream(s);
            double *o = out7 + 7 * (size_t) s;
            for (int k = 0; k < 7; k++) o[k] = 0;
            wins.emplace_back(new VisualWindow(S.camera, S.objectMap(), pbc, td, reprojection_error_std));
            VisualWindow &win = *wins.back();
            win.build();
            o[0] = win.numKeyFrames(), o[1] = win.numFactors();
            if (win.numKeyFrames() < 2 || win.numFactors() == 0) continue;
            priors[(size_t) s].resize((size_t) win.numKeyFrames());
            for (int k = 0; k < win.numKeyFrames(); k++) priors[(size_t) s][(size_t) k].assign(win.pose(k), win.pose(k) + 7);
            if (lockstep) {
                slot[(size_t) s] = batch.addWindow();
                win.addTo(batch, slot[(size_t) s]);
                const OnBatchWindow on{batch, slot[(size_t) s]};
                for (int k = 0; k < win.numKeyFrames(); k++) pose_prior(on, win.pose(k), priors[(size_t) s][(size_t) k].data(), prior_weight);
            } else {
                WindowSolver solver(win.batch(), 1.0);
                win.addTo(solver);
                for (int k = 0; k < win.numKeyFrames(); k++) pose_prior(solver, win.pose(k), priors[(size_t) s][(size_t) k].data(), prior_weight);
                WindowSolver::Options opt;
                WindowSolver::Summary s1, s2;
                opt.max_num_iterations = iters1;
                if (!solver.solve(opt, &s1)) {
                    set_err(err, errlen, solver.error().c_str());
                    return -2;
                }
                o[2] = s1.initial_cost, o[3] = s1.final_cost;
                if (chi2 > 0) {
                    o[4] = solver.removeReprojectionFactorsByChi2(chi2);
                    opt.max_num_iterations = iters2;
                    if (!solver.solve(opt, &s2)) {
                        set_err(err, errlen, solver.error().c_str());
                        return -3;
                    }
                    o[3] = s2.final_cost;
                }
            }
        }
        if (lockstep && batch.numWindows() > 0) {
            WindowSolverBatch::Options opt;
            vector<WindowSolverBatch::Summary> s1, s2;
            opt.max_num_iterations = iters1;
            if (!batch.solve(opt, &s1)) {
                set_err(err, errlen, batch.error().c_str());
                return -2;
            }
            vector<int> removed((size_t) batch.numWindows(), 0);
            if (chi2 > 0) {
                removed                = batch.removeReprojectionFactorsByChi2(chi2);
                opt.max_num_iterations = iters2;
                if (!batch.solve(opt, &s2)) {
                    set_err(err, errlen, batch.error().c_str());
                    return -3;
                }
            }
            for (int s = 0; s < n; s++) {
                if (slot[(size_t) s] < 0) continue;
                double *o = out7 + 7 * (size_t) s;
                const size_t w = (size_t) slot[(size_t) s];
                o[2] = s1[w].initial_cost, o[3] = chi2 > 0 ? s2[w].final_cost : s1[w].final_cost, o[4] = removed[w];
            }
        }
        // write-back and culling (all streams' observations in one launch)
        vector<WindowCulling::Stream> cull;
        vector<int> cull_stream;
        for (int s = 0; s < n; s++) {
            if (wins[(size_t) s]->numKeyFrames() < 2 || wins[(size_t) s]->numFactors() == 0) continue;
            wins[(size_t) s]->updateParametersFromOptimizer();
            cull.push_back(culling_stream(b, s, &wins[(size_t) s]->invdepthlist()));
            cull_stream.push_back(s);
        }
        vector<CullingResult> R;
        std::string e;
        if (!cull.empty() && !cull_by_context(b, cull, cull_stream, R, &e, [&](icg_ctx *c, const vector<WindowCulling::Stream> &part, vector<CullingResult> &r, std::string *pe) {
                return WindowCulling::gvinsOutlierCulling(c, part, reprojection_error_std, r, pe);
            })) {
            set_err(err, errlen, e.c_str());
            return -4;
        }
        for (size_t k = 0; k < cull_stream.size(); k++) {
            double *o = out7 + 7 * (size_t) cull_stream[k];
            o[5] = R[k].outlier_mappoints, o[6] = R[k].outlier_features;
        }
        if (kf_out)
            for (int s = 0; s < n; s++)
                for (int k = 0; k < std::min(max_kf, wins[(size_t) s]->numKeyFrames()); k++) {
                    double *r = kf_out + 14 * ((size_t) s * max_kf + k);
                    r[0] = wins[(size_t) s]->frame(k)->stamp(), r[1] = (double) wins[(size_t) s]->frame(k)->id();
                    Pose p = wins[(size_t) s]->frame(k)->pose();
                    poseToArray12(p, r + 2);
                }
        views.commit(); // (track-table engine: the write-back and the culling go into the table)
        return 0;
    });
}

} // extern "C"
