// The reprojection factors of many windows as ONE device factor set: what WindowSolverBatch (solver_batch_hip.h) and MarginalizationBatch
// (marg_batch.h) both put under the *_windows calls of the C ABI — the image-less back-end context, the per-window factor records with the
// window partition, their upload, the parameter gather, and the host threads of the per-window phases.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/icgvins_hip.h"
#include "host_pool.h"

namespace icg {

// Widest reduced system of the device path: the assembly (csrc/reproj_asm.hip k_asm_*) keeps no per-window tile in LDS any more — rounds 2-5
// held the camera block there (82, then 138 columns).  The reduction kernel k_schur_reduce_w stages its landmark rows of 4 ceil(P/4)
// doubles in SCH_PRE * 256 = 3 072 elements per pass (at least one row up to P = 3 072) and keeps two entries of s per thread (t and
// t + 256): P <= 512.  A window that can exceed it is the caller's to solve on the host.
constexpr int kMaxCameraColumns = 512;

// a context that holds no images (64 x 64, one slot); throws std::runtime_error("<who>: <the C ABI's message>")
icg_ctx *backendContext(int device, const char *who);

class WindowFactorSet {
public:
    struct Window {
        std::vector<double> obs;                   // 15 per factor, factor-major
        std::vector<int32_t> idx_i, idx_j, idx_lm; // window-local pose / landmark indices
        std::vector<double *> poses, landmarks;    // first-seen order of the factors
        std::unordered_map<const double *, int> pose_index, lm_index;
        double *ext{nullptr}, *td{nullptr};
        int fac_begin{0}, pose_begin{0}, lm_begin{0}; // the window's place in the factor set (upload())
        int size() const { return (int) (obs.size() / 15); }
    };

    // host_threads: 0 = hardware concurrency, at most 16; ICG_SOLVER_THREADS overrides either (diagnostics)
    WindowFactorSet(int device, int host_threads, const char *who);
    ~WindowFactorSet();
    WindowFactorSet(const WindowFactorSet &)            = delete;
    WindowFactorSet &operator=(const WindowFactorSet &) = delete;

    icg_ctx *ctx() const { return ctx_; }
    int addWindow();
    size_t numWindows() const { return windows_.size(); }
    const Window &window(size_t w) const { return windows_.at(w); }
    // a factor of window w: its 15 observation constants and its five blocks.  false (nothing added): the window already has another
    // extrinsic or td block
    bool add(int w, const double *obs15, double *pose_i, double *pose_j, double *ext, double *invdepth, double *td);
    // the factors of all windows, sorted by window, and the partition the *_windows calls work on.  Without any factor nothing is uploaded
    // (numFactors() == 0: the caller's to judge)
    bool upload(std::string *error);
    int numFactors() const { return n_factors_; }
    int numPoses() const { return n_poses_; }
    int numLandmarks() const { return n_lm_; }
    // the parameter blocks as icg_reproj_eval_windows takes them (a window without factors: an identity extrinsic nobody reads)
    void gather(std::vector<double> &poses, std::vector<double> &ext, std::vector<double> &inv, std::vector<double> &td);
    // drops every window, keeps the context and the threads
    void clear();

    // fn(w), w < n, on the persistent helper threads (created on first use: a batch of one or two windows never needs them).  The per-window
    // host phases take tens of microseconds per window: spawning threads per phase cost more than the phases themselves.
    template <typename F> void forEachWindow(size_t n, F &&fn) {
        if (host_threads_ <= 1 || n < 4) {
            for (size_t w = 0; w < n; w++) fn(w);
            return;
        }
        if (!pool_) pool_.reset(new HostPool(host_threads_));
        const std::function<void(int)> f = [&](int w) { fn((size_t) w); };
        pool_->parallelFor((int) n, f);
    }

private:
    icg_ctx *ctx_{nullptr};
    int host_threads_{1};
    std::unique_ptr<HostPool> pool_;
    std::vector<Window> windows_;
    int n_factors_{0}, n_poses_{0}, n_lm_{0};
};

} // namespace icg
