// The staged front-end both host engines run: the reference's per-frame algorithm (ic_gvins/ic_gvins/tracking/tracking.cc:144-245 and
// what it calls) cut into *stages* separated by the device calls (preprocess -> [detect] -> LK fwd/bwd -> RANSAC -> triangulate ->
// detect), so that `TrackingBatch` can run many independent camera streams in lock-step and hand ONE batched launch per stage to the GPU.
//
// StagedTracker<Engine, FrameRef> owns the state machine, the candidate lists and everything else that does not depend on how a frame
// and its features are stored.  An engine — icg::Tracking (object graph, tracking.h) or icg::TableTracker (track table, track_table.h) —
// derives from it (CRTP: every hook is a direct, inlinable call) and supplies
//   * the frame reference (Frame::Ptr / int handle): nullFrame(), frameCur() frameRef() framePre() frameLastKey() as lvalues, and per
//     frame numFeatures() stamp() pose() deviceSlot() setDeviceSlot() setKeyFrame() forEachKeyPoint();
//   * setPending() / takePending() / dropPending() for the frame handed to beginFrame(), isWindowFull(), bumpTrackedUsedTimes();
//   * detectionScratch() / detectionIntegrated() / clearCandidateHints() / afterStage() and the StageScope section timer;
//   * the list-building bodies, where the engines earn their difference: queueDetectionJob, queueTrackMappoint, finishTrackMappoint,
//     queueTrackReference, midTrackReference, finishTrackReference, queueTriangulation, finishTriangulation,
//     parallaxFromReferenceMapPoints.
// The tracker core (track_core.h) is a third statement of the same algorithm and stays its own text: lane-parallel code over a flat block.
#pragma once
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "hostprof.h"
#include "model.h"

namespace icg {

typedef enum TrackState { TRACK_FIRST_FRAME, TRACK_INITIALIZING, TRACK_TRACKING, TRACK_PASSED, TRACK_LOST } TrackState;

// tracker keys of config/gvins.yaml:48-57 (+ is_use_visualization :44)
struct TrackingConfig {
    bool track_check_histogram{false};
    double track_min_parallax{20};
    int track_max_features{200};
    double track_max_interval{0.5};
    bool is_use_visualization{false};
    double reprojection_error_std{1.5};
    static bool fromYamlFile(const std::string &path, TrackingConfig &cfg, std::string *err = nullptr);
};

// One stage worth of device work gathered from any number of streams.
struct StageBatch {
    // F1 preprocess
    vector<int32_t> pre_slots;
    vector<const uint8_t *> pre_imgs;
    int pre_stride{0}, pre_channels{1};
    bool pre_device{false};
    bool pre_want_hist{false};
    vector<double> pre_hist;
    // F7 detect
    vector<int32_t> det_slots, det_mask_off{0}, det_quota;
    vector<float> det_mask_pts;
    vector<float> det_out;
    vector<int32_t> det_count;
    // F2/F3 LK forward-backward (+F4 undistort)
    vector<int32_t> lk_prev_slot, lk_next_slot;
    vector<float> lk_prev, lk_guess, lk_out, lk_undist;
    vector<uint8_t> lk_status;
    // camera index per LK point into the context's camera table (DeviceContext::setCameras): filled by TrackingBatch::gather with the
    // stream's local index, empty in a single stream's own batch
    vector<int32_t> lk_cam;
    // lk_base: where this stream's points start in the concatenated call (set when results are split back)
    int lk_base{0};
    // F6 RANSAC
    vector<int32_t> rs_off{0};
    vector<float> rs_p1, rs_p2;
    vector<uint8_t> rs_mask;
    double rs_thresh{1.5}, rs_conf{0.99}; // reprojection_error_std_, 0.99 (tracking.cc:548)
    // F8 triangulate
    vector<int32_t> tri_T0, tri_T1;
    vector<double> tri_Tcw, tri_pc0, tri_pc1, tri_pw;
    void clear();
};

// Thin RAII wrapper over icg_ctx with the stage executor.
class DeviceContext {
public:
    typedef std::shared_ptr<DeviceContext> Ptr;
    DeviceContext(int device, int width, int height, int n_streams, int max_features);
    ~DeviceContext();
    icg_ctx *ctx() { return ctx_; }
    void setCamera(const Camera &cam);
    // One camera per stream of the context (icg_set_cameras): execute() then undistorts every LK point with the camera StageBatch::lk_cam
    // names.  A table of bit-equal cameras is the single camera (setCamera) and sets no table.  A build of this layer on an implementation
    // of the C ABI without the camera-table entries refuses a heterogeneous table by name (std::runtime_error).
    void setCameras(const vector<Camera::Ptr> &cams);
    int cameraTableSize() const { return n_cams_; } // 0: single camera
    static bool sameCameras(const vector<Camera::Ptr> &cams);
    // runs whatever the batch contains, one ABI call per kind of work; throws std::runtime_error on ABI failure
    void execute(StageBatch &b, const icg_detect_grid &grid, int max_per_job);
    int allocSlot();
    void freeSlot(int s);
    // Kernel-only replay (profiles/r03_kernel_ceiling.json): while recording, every execute() keeps a copy of its work lists; replay()
    // issues the recorded calls again, back to back, with no tracker logic in between — under icg_prof_enable that yields the exclusive
    // device time of every kernel of a step.  Valid until the next frame is tracked (the frame slots still hold the recorded images).
    void record(bool on) {
        recording_ = on;
        if (on) recorded_.clear();
    }
    size_t recorded() const { return recorded_.size(); }
    // `first`: index of the recorded call to start with (the calls of a step only depend on the frame slots, not on each other, so a replay
    // may start anywhere: concurrent replays of several contexts are staggered that way, as free-running groups are)
    void replay(const icg_detect_grid &grid, int max_per_job, size_t first = 0) {
        for (size_t k = 0; k < recorded_.size(); k++) {
            StageBatch copy = recorded_[(first + k) % recorded_.size()];
            const bool was = recording_;
            recording_     = false;
            execute(copy, grid, max_per_job);
            recording_ = was;
        }
    }

private:
    bool recording_{false};
    vector<StageBatch> recorded_;
    icg_ctx *ctx_{nullptr};
    int n_cams_{0};
    vector<int> free_slots_;
    std::mutex slot_mutex_;
};

// The detection grid and feature quotas of a camera (tracking.cc:57-85)
struct TrackGeometry {
    int block_cols, block_rows, block_cnts, block_w, block_h;
    int max_block_features, min_pixel_distance, max_per_job;
    double track_max_interval; // x 0.95 (:57)
    icg_detect_grid grid;
};

inline TrackGeometry trackGeometry(const Camera &camera, const TrackingConfig &cfg) {
    const double TRACK_BLOCK_SIZE = 200.0; // tracking.h:112
    TrackGeometry g;
    g.track_max_interval = cfg.track_max_interval * 0.95; // :57
    g.block_cols = static_cast<int>(lround(camera.width() / TRACK_BLOCK_SIZE));  // :66
    g.block_rows = static_cast<int>(lround(camera.height() / TRACK_BLOCK_SIZE)); // :67
    g.block_cnts = g.block_cols * g.block_rows;
    g.block_h    = camera.height() / g.block_rows; // :71
    g.block_w    = camera.width() / g.block_cols;  // :72
    g.max_block_features = static_cast<int>(lround(static_cast<double>(cfg.track_max_features) / static_cast<double>(g.block_cnts))); // :81
    g.min_pixel_distance = static_cast<int>(round(TRACK_BLOCK_SIZE / sqrt(g.max_block_features * 1.5)));                             // :85
    g.max_per_job        = g.max_block_features * g.block_cnts;
    g.grid               = icg_detect_grid{};
    g.grid.block_cols    = g.block_cols;
    g.grid.block_rows    = g.block_rows;
    g.grid.block_w       = g.block_w;
    g.grid.block_h       = g.block_h;
    g.grid.min_dist      = g.min_pixel_distance;
    g.grid.max_per_block = g.max_block_features;
    return g;
}

// One line of tracking.txt (tracking.cc:309-315): the five numbers of the keyframe decision, the feature count and the time cost, in
// FileSaver's text format "%-15.9lf " per value (fileio/filesaver.cc:51-66)
inline void writeTrackingLine(FILE *f, const double data5[5], int features, double cost_ms) {
    for (int k = 0; k < 5; k++) fprintf(f, "%-15.9lf ", data5[k]);
    fprintf(f, "%-15.9lf %-15.9lf \n", static_cast<double>(features), cost_ms);
    fflush(f);
}

template <class Engine, class FrameRef> class StagedTracker {
public:
    enum { N_STAGES = 7 };
    const icg_detect_grid &grid() const { return grid_; }
    int maxFeaturesPerJob() const { return grid_.max_per_block * block_cnts_; }

protected:
    StagedTracker(Camera::Ptr camera, const TrackingConfig &config, DeviceContext::Ptr device, std::shared_ptr<IdSpace> ids)
        : cfg_(config), camera_(std::move(camera)), device_(std::move(device)), ids_(std::move(ids)),
          host_check_(getenv("ICG_HOST_CHECK") != nullptr), det_frame_(Engine::nullFrame()) {
        const TrackGeometry g     = trackGeometry(*camera_, cfg_);
        block_cols_               = g.block_cols;
        block_cnts_               = g.block_cnts;
        block_w_                  = g.block_w;
        block_h_                  = g.block_h;
        track_max_block_features_ = g.max_block_features;
        track_max_interval_       = g.track_max_interval;
        grid_                     = g.grid;
    }
    ~StagedTracker() {
        if (logfile_) fclose(logfile_);
        for (int s : owned_slots_) device_->freeSlot(s);
        if (pending_slot_ >= 0) device_->freeSlot(pending_slot_);
    }
    StagedTracker(const StagedTracker &)            = delete;
    StagedTracker &operator=(const StagedTracker &) = delete;

    void openLog(const std::string &outputpath) { // :44-50; the reference logs an error and leaves the tracker half-constructed, this one throws
        if (outputpath.empty()) return;
        logfile_ = fopen((outputpath + "/tracking.txt").c_str(), "w");
        if (!logfile_) throw std::runtime_error("Tracking: failed to open " + outputpath + "/tracking.txt");
    }

    // ---- helpers ---------------------------------------------------------------------------------------------------
    template <typename T> static void reduceVector(T &vec, const vector<uint8_t> &status) { // :831-839
        size_t index = 0;
        for (size_t k = 0; k < vec.size(); k++)
            if (status[k]) {
                if (index != k) vec[index] = std::move(vec[k]); // (shared_ptr lists: no reference-count round trip per kept element)
                index++;
            }
        vec.resize(index);
    }

    bool isOnBorder(const Point2f &pts) const { // :847-849
        return pts.x < 5.0 || pts.y < 5.0 || (pts.x > (camera_->width() - 5.0)) || (pts.y > (camera_->height() - 5.0));
    }

    static bool isGoodDepth(double depth, double scale = 1.0) { // :247-249
        return ((depth > MapPoint::NEAREST_DEPTH) && (depth < MapPoint::FARTHEST_DEPTH * scale));
    }

    bool isGoodToTrack(const Point2f &pp, const Pose &pose, const Vector3d &pw, double scale, double depth_scale = 1.0) { // :813-829
        Vector3d pc = Camera::world2cam(pw, pose);
        if (!isGoodDepth(pc[2], depth_scale)) return false;
        if (camera_->reprojectionError(pose, pw, pp).norm() > cfg_.reprojection_error_std * scale) return false;
        return true;
    }

    double keyPointParallax(const Point2f &pp0, const Point2f &pp1, const Pose &pose0, const Pose &pose1) { // :861-871
        Vector3d pc0  = camera_->pixel2cam(pp0);
        Vector3d pc1  = camera_->pixel2cam(pp1);
        Vector3d pc01 = (pose1.R.transpose() * pose0.R) * pc0;
        return Vector2d(pc01[0] - pc1[0], pc01[1] - pc1[1]).norm() * camera_->focalLength();
    }

    double keyPointParallax(const Point2f &pp0, const Point2f &pp1, const Matrix3d &R10) { // R10 = pose1.R^T * pose0.R
        Vector3d pc0  = camera_->pixel2cam(pp0);
        Vector3d pc1  = camera_->pixel2cam(pp1);
        Vector3d pc01 = R10 * pc0;
        return Vector2d(pc01[0] - pc1[0], pc01[1] - pc1[1]).norm() * camera_->focalLength();
    }

    // ICG_HOST_CHECK=1 (read when the tracker is built): the carried undistorted twins must equal a fresh Camera::undistortPoints of
    // their sources, bit for bit
    void checkCarriedUndistortion(const char *where) {
        if (!host_check_) return;
        auto same = [&](const vector<Point2f> &src, const vector<Point2f> &carried, const char *what) {
            if (src.size() != carried.size())
                throw std::runtime_error(std::string("carried undistortion size mismatch (") + what + ") at " + where);
            vector<Point2f> u = src;
            camera_->undistortPoints(u);
            for (size_t k = 0; k < u.size(); k++)
                if (memcmp(&u[k], &carried[k], sizeof(Point2f)) != 0)
                    throw std::runtime_error(std::string("carried undistortion differs (") + what + ") at " + where);
        };
        same(pts2d_ref_, pts2d_ref_undis_, "ref");
        if (where[0] == 't' && where[2] == 'i') // "triangulation": pts2d_new_ is stale here, pts2d_cur_ is live
            same(pts2d_cur_, tr_cur_undis_, "cur");
        else
            same(pts2d_new_, pts2d_new_undis_, "new");
    }

    int parallaxFromReferenceKeyPoints(const vector<Point2f> &ref, const vector<Point2f> &cur, double &parallax) { // :907-922
        parallax   = 0;
        int counts = 0;
        const Matrix3d R10 = self().pose(self().frameCur()).R.transpose() * self().pose(self().frameRef()).R;
        for (size_t k = 0; k < pts2d_ref_frame_.size(); k++) {
            if (pts2d_ref_frame_[k] == self().frameRef()) {
                parallax += keyPointParallax(ref[k], cur[k], R10);
                counts++;
            }
        }
        if (counts != 0) parallax /= counts;
        return counts;
    }

    double relativeTranslation() { return (self().pose(self().frameCur()).t - self().pose(self().frameRef()).t).norm(); } // :331-333

    double relativeRotation() { // :335-341 (Rotation::matrix2euler pitch component, common/rotation.h:47)
        Matrix3d R   = self().pose(self().frameCur()).R.transpose() * self().pose(self().frameRef()).R;
        double pitch = atan(-R(2, 0) / sqrt(R(2, 1) * R(2, 1) + R(2, 2) * R(2, 2)));
        return fabs(pitch * (180.0 / M_PI));
    }

    bool doResetTracking() { // :317-329
        if (!self().numFeatures(self().frameCur())) {
            isinitializing_  = true;
            self().frameRef() = self().frameCur();
            clearCandidates();
            return true;
        }
        return false;
    }

    void clearCandidates() {
        pts2d_new_.clear();
        pts2d_ref_.clear();
        pts2d_ref_undis_.clear();
        pts2d_new_undis_.clear();
        pts2d_ref_frame_.clear();
        velocity_ref_.clear();
        self().clearCandidateHints();
    }

    void writeLoggingMessage() { // :309-315
        if (!logfile_) return;
        writeTrackingLine(logfile_, logging_data_.data(), (int) self().numFeatures(self().frameCur()),
                          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start_).count());
    }

    keyFrameState checkKeyFrameSate() { // :263-307
        keyFrameState keyframe_state = KEYFRAME_NONE;
        double dt                    = self().stamp(self().frameCur()) - self().stamp(self().frameLastKey());
        if (dt < TRACK_MIN_INTERVAl) return keyframe_state;
        double parallax = (parallax_map_ * parallax_map_counts_ + parallax_ref_ * parallax_ref_counts_) /
                          (parallax_map_counts_ + parallax_ref_counts_);
        if (parallax > cfg_.track_min_parallax) {
            keyframe_state = self().isWindowFull() ? KEYFRAME_REMOVE_OLDEST : KEYFRAME_NORMAL;
        } else if (dt > track_max_interval_) {
            keyframe_state = KEYFRAME_REMOVE_SECOND_NEW;
        }
        if (keyframe_state != KEYFRAME_NONE) {
            self().frameLastKey() = self().frameCur();
            self().bumpTrackedUsedTimes();
            logging_data_.clear();
            logging_data_.push_back(self().stamp(self().frameCur()));
            logging_data_.push_back(dt);
            logging_data_.push_back(parallax);
            logging_data_.push_back(relativeTranslation());
            logging_data_.push_back(relativeRotation());
        }
        return keyframe_state;
    }

    // ---- device slots: at most {ref, pre, cur, incoming} are resident per stream ----------------------------------------
    void assignSlot(const FrameRef &f) {
        self().setDeviceSlot(f, pending_slot_);
        owned_slots_.push_back(pending_slot_);
        pending_slot_ = -1;
    }

    void releaseUnusedSlots() {
        auto holds = [&](const FrameRef &f, int s) { return !(f == Engine::nullFrame()) && self().deviceSlot(f) == s; };
        size_t keep = 0;
        for (int s : owned_slots_) {
            if (holds(self().frameCur(), s) || holds(self().framePre(), s) || holds(self().frameRef(), s))
                owned_slots_[keep++] = s;
            else
                device_->freeSlot(s);
        }
        owned_slots_.resize(keep);
    }

    // ---- stage 0: preprocessing (tracking.cc:107-142) ------------------------------------------------------------------
    // `in` is what the engine tracks a frame from (Frame::Ptr / TableTracker::Input); setPending() keeps it and returns its image
    template <typename In> void beginFrame(In &&in, StageBatch &next) {
        t_start_       = std::chrono::steady_clock::now(); // timecost_.restart() :147
        done_          = false;
        result_        = TRACK_PASSED;
        isnewkeyframe_ = false; // :108
        mode_          = M_NONE;
        det_job_       = -1;
        rs_set_        = -1;
        tri_queued_    = false;
        lk_map_n_ = lk_ref_n_ = 0;
        ref_tracked_   = false;
        const Mat &img = self().setPending(std::forward<In>(in));
        pending_slot_  = device_->allocSlot();
        next.pre_slots.push_back(pending_slot_);
        next.pre_imgs.push_back(img.data);
        next.pre_stride   = (int) img.step;
        next.pre_channels = img.channels(); // BGR->gray on device (:111-113)
        next.pre_device   = img.device;
        if (cfg_.track_check_histogram) next.pre_want_hist = true;
        // remember which job is ours
        det_job_ = (int) next.pre_slots.size() - 1; // reused as "preprocess job index" until stage 1
    }

    void advance(int stage, StageBatch &done, StageBatch &next) { // stage 1..6
        if (done_) return;
        switch (stage) {
        case 1: onPreprocessDone(done, next); break;
        case 2: onDetectADone(done, next); break;
        case 3: onLKDone(done, next); break;
        case 4: onRansacDone(done, next); break;
        case 5: onTriangulateDone(done, next); break;
        case 6: onDetectBDone(done); break;
        default: break;
        }
    }

    void finish(TrackState st) {
        result_ = st;
        done_   = true;
    }

    void onPreprocessDone(StageBatch &done, StageBatch &next) {
        if (cfg_.track_check_histogram) { // :115-133
            double hist = done.pre_hist[(size_t) det_job_];
            if (histogram_ != 0) {
                double rate = fabs((hist - histogram_) / histogram_);
                if (rate > 0.1) {
                    passed_cnt_++;
                    if (passed_cnt_ > 1) histogram_ = 0;
                    device_->freeSlot(pending_slot_);
                    pending_slot_ = -1;
                    self().dropPending();
                    finish(TRACK_PASSED);
                    return;
                }
            }
            histogram_ = hist;
        }
        det_job_           = -1;
        self().framePre() = self().frameCur(); // :135
        self().frameCur() = self().takePending();
        assignSlot(self().frameCur());
        releaseUnusedSlots();

        if (isinitializing_) {
            if (self().frameRef() == Engine::nullFrame()) { // :158-166
                doResetTracking();
                self().frameRef() = self().frameCur();
                mode_             = M_FIRST;
                queueDetection(self().frameRef(), false, next);
                return;
            }
            mode_ = M_INIT;
            if (pts2d_ref_.empty()) queueDetection(self().frameRef(), false, next); // :168-170
        } else {
            mode_ = M_TRACK;
        }
    }

    void onDetectADone(StageBatch &done, StageBatch &next) {
        if (det_job_ >= 0) {
            typename Engine::StageScope hp(hostprof::DET_INTEGRATE);
            integrateDetection(done);
        }
        if (mode_ == M_FIRST) {
            releaseUnusedSlots();
            finish(TRACK_FIRST_FRAME);
            return;
        }
        if (mode_ == M_TRACK) { // :206
            typename Engine::StageScope hp(hostprof::QUEUE_MAP);
            self().queueTrackMappoint(next);
        }
        typename Engine::StageScope hp(hostprof::QUEUE_REF);
        self().queueTrackReference(next); // :173 / :209
    }

    void onLKDone(StageBatch &done, StageBatch &next) {
        if (mode_ == M_TRACK) self().finishTrackMappoint(done);
        ref_tracked_ = self().midTrackReference(done, next);
    }

    void onRansacDone(StageBatch &done, StageBatch &next) {
        if (ref_tracked_) self().finishTrackReference(done);
        if (mode_ == M_INIT) {
            if (parallax_ref_ < cfg_.track_min_parallax) { // :175-178
                self().afterStage();
                finish(TRACK_INITIALIZING);
                return;
            }
            self().queueTriangulation(next); // :182
            return;
        }
        kf_state_ = checkKeyFrameSate(); // :212
        if ((kf_state_ == KEYFRAME_NORMAL) || (kf_state_ == KEYFRAME_REMOVE_OLDEST)) self().queueTriangulation(next); // :215-217
    }

    void onTriangulateDone(StageBatch &done, StageBatch &next) {
        if (tri_queued_) self().finishTriangulation(done);
        if (mode_ == M_INIT) {
            if (doResetTracking()) { // :184-190
                self().afterStage();
                lost_reset_ = 1;
                makeNewFrameQueue(KEYFRAME_NORMAL, next);
                return;
            }
            lost_reset_ = 0;
            self().setKeyFrame(self().frameRef(), KEYFRAME_NORMAL); // :193
            makeNewFrameQueue(KEYFRAME_NORMAL, next);               // :196
            self().frameLastKey() = self().frameCur();
            isinitializing_       = false;
            return;
        }
        // tracking mode (:214-239). featuresDetection never touches frame features, so the lost test (:224) can be
        // evaluated first: when it fires the results of the :220 detection would be wiped by doResetTracking anyway.
        lost_reset_ = 0;
        if (!self().numFeatures(self().frameCur())) {
            doResetTracking();
            lost_reset_ = 2;
            makeNewFrameQueue(KEYFRAME_NORMAL, next); // :225
            return;
        }
        if ((kf_state_ == KEYFRAME_NORMAL) || (kf_state_ == KEYFRAME_REMOVE_OLDEST)) {
            makeNewFrameQueue(kf_state_, next); // :230-232
        } else {
            queueDetection(self().frameCur(), true, next); // :220
            if (kf_state_ != KEYFRAME_NONE) makeNewFrameQueue(kf_state_, next); // REMOVE_SECOND_NEW: flags only
        }
    }

    void onDetectBDone(StageBatch &done) {
        if (det_job_ >= 0) integrateDetection(done);
        releaseUnusedSlots();
        if (mode_ == M_INIT) {
            if (lost_reset_ == 1) {
                finish(TRACK_FIRST_FRAME);
                return;
            }
            self().afterStage();
            finish(TRACK_TRACKING);
            return;
        }
        if (lost_reset_ == 2) {
            finish(TRACK_LOST);
            return;
        }
        if (kf_state_ != KEYFRAME_NONE) writeLoggingMessage(); // :236-238
        self().afterStage();
        finish(TRACK_TRACKING);
    }

    // makeNewFrame (:251-261) with its detection deferred to the batched stage
    void makeNewFrameQueue(int state, StageBatch &next) {
        self().setKeyFrame(self().frameCur(), state);
        isnewkeyframe_ = true;
        if ((state == KEYFRAME_NORMAL) || (state == KEYFRAME_REMOVE_OLDEST)) {
            self().frameRef() = self().frameCur();
            queueDetection(self().frameRef(), true, next);
        }
    }

    // ---- featuresDetection (:576-688) ------------------------------------------------------------------------------------
    bool queueDetection(const FrameRef &frame, bool ismask, StageBatch &next) {
        det_job_ = -1;
        int num_features = static_cast<int>(self().numFeatures(frame) + pts2d_ref_.size()); // :579
        if (num_features > (cfg_.track_max_features - 5)) return false;                     // :580
        self().queueDetectionJob(frame, ismask, next);
        return true;
    }

    // features_cnts[block_cnts_] := key points of `frame` and candidates per detection block (:590-608)
    void countBlockFeatures(const FrameRef &frame, int *features_cnts) {
        for (int k = 0; k < block_cnts_; k++) features_cnts[k] = 0;
        auto count = [&](float x, float y) {
            int col = int(x / (float) block_w_); // :598
            int row = int(y / (float) block_h_);
            // SURVEY.md hazard H5: the reference indexes features_cnts[row * block_cols_ + col] with the UNCLAMPED column.  The key
            // points counted here are undistorted, so near the right edge x can reach block_cols_ * block_w_ and beyond
            // (col == block_cols_): the reference then counts the feature in the FIRST block of the NEXT row.  That effective
            // behaviour is reproduced (pinned by tests/golden/tracking_ref_*.npz); only indices outside the array — undefined
            // behaviour in the reference (stack VLA overrun) — are dropped.
            const long idx = (long) row * block_cols_ + col;
            if (idx >= 0 && idx < (long) block_cnts_) features_cnts[idx]++;
        };
        self().forEachKeyPoint(frame, count);
        for (auto &pts2d : pts2d_new_) count(pts2d.x, pts2d.y);
    }

    void integrateDetection(StageBatch &done) { // :659-685
        if (!det_ismask_) clearCandidates();
        const int max_per_job = maxFeaturesPerJob();
        const int n           = done.det_count[(size_t) det_job_];
        const float *p        = done.det_out.data() + (size_t) det_job_ * max_per_job * 2;
        auto scratch                 = self().detectionScratch();
        vector<Point2f> &fresh       = scratch.a;
        vector<Point2f> &fresh_undis = scratch.b;
        fresh.resize((size_t) n);
        for (int i = 0; i < n; i++) fresh[(size_t) i] = Point2f(p[2 * i], p[2 * i + 1]);
        fresh_undis = fresh;
        camera_->undistortPoints(fresh_undis); // the one undistortion a detected corner ever needs
        for (int i = 0; i < n; i++) {
            pts2d_ref_.push_back(fresh[(size_t) i]);
            pts2d_new_.push_back(fresh[(size_t) i]);
            pts2d_ref_undis_.push_back(fresh_undis[(size_t) i]);
            pts2d_new_undis_.push_back(fresh_undis[(size_t) i]);
            pts2d_ref_frame_.push_back(det_frame_);
            velocity_ref_.emplace_back(0, 0);
        }
        self().detectionIntegrated(n);
        det_job_   = -1;
        det_frame_ = Engine::nullFrame();
    }

    void afterStage() {} // default hook: nothing to show

protected:
    static constexpr int TRACK_PYRAMID_LEVEL   = 3;    // tracking.h:113
    static constexpr double TRACK_MIN_PARALLAX = 10.0; // tracking.h:114
    static constexpr double TRACK_MIN_INTERVAl = 0.08; // tracking.h:115

    TrackingConfig cfg_;
    Camera::Ptr camera_;
    DeviceContext::Ptr device_;
    std::shared_ptr<IdSpace> ids_;
    const bool host_check_;

    // candidates (tracking.h:129-136)
    vector<Point2f> pts2d_cur_, pts2d_new_, pts2d_ref_;
    // undistorted twins of pts2d_ref_ / pts2d_new_, carried through every reduceVector instead of re-running
    // Camera::undistortPoints on unchanged points each frame (tracking.cc:469,520-524,542-544,712-713): a reference point
    // is undistorted once when detected / re-anchored, and a tracked point's undistorted position comes back from the LK
    // kernel (same iteration, bit-identical; ICG_HOST_CHECK=1 re-derives them on the host and compares)
    vector<Point2f> pts2d_ref_undis_, pts2d_new_undis_;
    vector<FrameRef> pts2d_ref_frame_;
    vector<Vector2d> velocity_ref_, velocity_cur_;

    int block_cols_, block_cnts_, block_w_, block_h_, track_max_block_features_;
    double track_max_interval_;
    icg_detect_grid grid_{};

    double parallax_map_{0}, parallax_ref_{0};
    int parallax_map_counts_{0}, parallax_ref_counts_{0};

    bool isnewkeyframe_{false};
    bool isinitializing_{true};
    double histogram_{0};
    int passed_cnt_{0};

    FILE *logfile_{nullptr};
    std::chrono::steady_clock::time_point t_start_;
    vector<double> logging_data_; // the five numbers of the last keyframe decision

    // ---- per-frame staged state ----
    bool done_{true};
    TrackState result_{TRACK_PASSED};
    int pending_slot_{-1};
    vector<int> owned_slots_; // slots currently holding pre/cur/ref images
    enum Mode { M_NONE, M_FIRST, M_INIT, M_TRACK } mode_{M_NONE};
    // detection job bookkeeping
    int det_job_{-1};
    bool det_ismask_{true};
    FrameRef det_frame_;
    // LK bookkeeping
    int lk_map_begin_{0}, lk_map_n_{0}, lk_ref_begin_{0}, lk_ref_n_{0};
    bool ref_tracked_{false};
    // RANSAC bookkeeping
    int rs_set_{-1};
    vector<Point2f> tr_new_undis_, tr_cur_undis_;
    // triangulation bookkeeping
    keyFrameState kf_state_{KEYFRAME_NONE};
    bool tri_queued_{false};
    int tri_begin_{0};
    vector<int> tri_point_index_; // k (index into pts2d_cur_) per queued point
    vector<uint8_t> tri_status_;  // final reduceVector status (size pts2d_cur_)
    vector<Point2f> tri_ref_undis_, tri_cur_undis_;
    int lost_reset_{0};

private:
    Engine &self() { return *static_cast<Engine *>(this); }
};

} // namespace icg
