// INS-aided KLT visual front-end on MI355X: the reference's `Tracking` API re-built on the C ABI of
// include/icgvins_hip.h (reference: ic_gvins/ic_gvins/tracking/tracking.h:46-169, tracking.cc).
//
// Public surface kept from the reference: Tracking(camera, map, drawer, configfile, outputpath), track(frame),
// isNewKeyFrame(), isGoodToTrack(...), pose2Tcw(pose), TrackState.  New: the per-frame algorithm runs as the *stages* of
// staged_tracker.h, which owns the state machine and the candidate lists; this class is its object-graph engine (Frame /
// Feature / MapPoint / Map objects, the drawer) and supplies the list-building bodies.  track(frame) simply runs the stages
// for a single stream.
#pragma once
#include "staged_tracker.h"

namespace icg {

class Tracking : public StagedTracker<Tracking, Frame::Ptr> {
    typedef StagedTracker<Tracking, Frame::Ptr> Base;
    friend Base;

public:
    typedef std::shared_ptr<Tracking> Ptr;

    // reference signature (tracking.h:51); configfile is the flat YAML of config/gvins.yaml
    Tracking(Camera::Ptr camera, Map::Ptr map, Drawer::Ptr drawer, const std::string &configfile, const std::string &outputpath);
    // same with an explicit configuration, a shared device context (several streams on one GPU) and an id space
    Tracking(Camera::Ptr camera, Map::Ptr map, Drawer::Ptr drawer, const TrackingConfig &config, const std::string &outputpath,
             DeviceContext::Ptr device, std::shared_ptr<IdSpace> ids = IdSpace::global());

    TrackState track(Frame::Ptr frame);
    bool isNewKeyFrame() const { return isnewkeyframe_; }
    using Base::isGoodToTrack; // (pp, pose, pw, scale, depth_scale = 1.0)
    static Matrix4d pose2Tcw(const Pose &pose);

    // ---- staged interface used by TrackingBatch (and by track()) ----
    void beginFrame(Frame::Ptr frame, StageBatch &next);           // stage 0: queue preprocess
    void advance(int stage, StageBatch &done, StageBatch &next);   // stage 1..6
    bool frameDone() const { return done_; }
    TrackState result() const { return result_; }
    const std::shared_ptr<IdSpace> &ids() const { return ids_; }
    size_t numTrackedRefPoints() const { return pts2d_new_.size(); }
    // the un-triangulated candidates carried to the next frame (tracking.h:129 pts2d_new_ / pts2d_ref_), for tests
    const vector<Point2f> &trackedRefPoints() const { return pts2d_new_; }
    const vector<Point2f> &referencePoints() const { return pts2d_ref_; }
    const Frame::Ptr &currentFrame() const { return frame_cur_; }
    const Frame::Ptr &referenceFrame() const { return frame_ref_; }
    // tracker state for engine-vs-engine tests (TableTracker::dumpObjects)
    const Frame::Ptr &previousFrame() const { return frame_pre_; }
    const Frame::Ptr &lastKeyFrame() const { return last_keyframe_; }
    const vector<Frame::Ptr> &referencePointFrames() const { return pts2d_ref_frame_; }
    const vector<Vector2d> &referenceVelocities() const { return velocity_ref_; }
    bool initializing() const { return isinitializing_; }
    double parallaxMap() const { return parallax_map_; }
    double parallaxRef() const { return parallax_ref_; }
    int parallaxMapCounts() const { return parallax_map_counts_; }
    int parallaxRefCounts() const { return parallax_ref_counts_; }

public:
    static constexpr double ASSOCIATE_MAXIUM_DISTANCE      = 1.0;
    static constexpr double ASSOCIATE_MAXIUM_DISTANCE_RATE = 0.05;
    static constexpr double ASSOCIATE_DEPTH_STD            = 0.1;

private:
    Tracking(Camera::Ptr camera, Map::Ptr map, Drawer::Ptr drawer, const TrackingConfig &config, const std::string &outputpath); // own device

    // ---- what the staged state machine asks of its engine (staged_tracker.h) ----
    static constexpr std::nullptr_t nullFrame() { return nullptr; }
    Frame::Ptr &frameCur() { return frame_cur_; }
    Frame::Ptr &frameRef() { return frame_ref_; }
    Frame::Ptr &framePre() { return frame_pre_; }
    Frame::Ptr &frameLastKey() { return last_keyframe_; }
    static size_t numFeatures(const Frame::Ptr &f) { return f->numFeatures(); }
    static double stamp(const Frame::Ptr &f) { return f->stamp(); }
    static Pose pose(const Frame::Ptr &f) { return f->pose(); }
    static int deviceSlot(const Frame::Ptr &f) { return f->deviceSlot(); }
    static void setDeviceSlot(const Frame::Ptr &f, int slot) { f->setDeviceSlot(slot); }
    static void setKeyFrame(const Frame::Ptr &f, int state) { f->setKeyFrame(state); }
    template <typename F> static void forEachKeyPoint(const Frame::Ptr &f, F &&fn) {
        f->forEachFeaturePipelined([&](ulong, const Feature::Ptr &feature) { fn(feature->keyPoint().x, feature->keyPoint().y); });
    }
    const Mat &setPending(Frame::Ptr frame) { return (pending_frame_ = std::move(frame))->image(); }
    Frame::Ptr takePending() { return std::move(pending_frame_); }
    void dropPending() { pending_frame_.reset(); }
    bool isWindowFull() { return map_->isWindowFull(); }
    void bumpTrackedUsedTimes() {
        for (auto &mappoint : tracked_mappoint_) mappoint->increaseUsedTimes();
    }
    struct FreshPoints {
        vector<Point2f> a, b;
    };
    static FreshPoints detectionScratch() { return {}; }
    void detectionIntegrated(int n);
    void clearCandidateHints() {}
    void afterStage() { showTracking(); }
    struct StageScope { // (the object engine times no sections of its stage bodies)
        explicit StageScope(int) {}
    };

    // the list-building bodies of the reference algorithm
    void queueDetectionJob(const Frame::Ptr &frame, bool ismask, StageBatch &next);
    void queueTrackMappoint(StageBatch &next);
    bool finishTrackMappoint(StageBatch &done);
    void queueTrackReference(StageBatch &next);
    bool midTrackReference(StageBatch &done, StageBatch &next);
    bool finishTrackReference(StageBatch &done);
    bool queueTriangulation(StageBatch &next);
    void finishTriangulation(StageBatch &done);
    int parallaxFromReferenceMapPoints(double &parallax);
    void showTracking();

private:
    Frame::Ptr frame_cur_, frame_ref_, frame_pre_, last_keyframe_, pending_frame_;
    Map::Ptr map_;
    Drawer::Ptr drawer_;
    vector<MapPoint::Ptr> tracked_mappoint_, mappoint_matched_;

    vector<Point2f> tm_pts2d_map_, tm_pts2d_map_undis_;
    vector<MapPointType> tm_type_;
    vector<int> tri_action_; // per k: 0 = decided early, 1 = needs device result
};

// Stand-in for the part of GVINS that owns the sliding window (ic_gvins.cc:724-747, 1391-1410, 440-448, 1675):
// inserts keyframes, drops REMOVE_SECOND_NEW / empty frames, removes the oldest keyframe with its landmarks when
// the window overflows.  Used by the replay/bench harness so the tracker sees a live window.
class WindowKeeper {
public:
    explicit WindowKeeper(Map::Ptr map) : map_(std::move(map)) {}
    void onFrame(Tracking &tracking, const Frame::Ptr &frame, TrackState st);

private:
    Map::Ptr map_;
};

} // namespace icg
