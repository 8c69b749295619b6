// WindowFactorSet: see window_factors.h.
#include "window_factors.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <thread>

namespace icg {

icg_ctx *backendContext(int device, const char *who) {
    icg_ctx_config cfg{};
    cfg.device = device, cfg.width = 64, cfg.height = 64, cfg.n_slots = 1, cfg.max_batch = 1, cfg.max_points = 64; // (holds no images)
    icg_ctx *ctx = nullptr;
    if (icg_ctx_create(&cfg, &ctx) != ICG_OK) throw std::runtime_error(std::string(who) + ": " + icg_last_error(nullptr));
    return ctx;
}

WindowFactorSet::WindowFactorSet(int device, int host_threads, const char *who) {
    host_threads_ = host_threads > 0 ? host_threads : (int) std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char *e = getenv("ICG_SOLVER_THREADS")) host_threads_ = std::max(1, atoi(e)); // diagnostics
    ctx_ = backendContext(device, who);
}

WindowFactorSet::~WindowFactorSet() { icg_ctx_destroy(ctx_); }

int WindowFactorSet::addWindow() {
    windows_.emplace_back();
    return (int) windows_.size() - 1;
}

void WindowFactorSet::clear() {
    windows_.clear();
    n_factors_ = n_poses_ = n_lm_ = 0;
}

bool WindowFactorSet::add(int w, const double *obs15, double *pose_i, double *pose_j, double *ext, double *invdepth, double *td) {
    Window &W = windows_.at((size_t) w);
    if ((W.ext && W.ext != ext) || (W.td && W.td != td)) return false;
    W.ext = ext, W.td = td;
    auto index_of = [](std::unordered_map<const double *, int> &m, std::vector<double *> &v, double *p) {
        auto it = m.find(p);
        if (it != m.end()) return it->second;
        const int k = (int) v.size();
        v.push_back(p);
        m[p] = k;
        return k;
    };
    W.obs.insert(W.obs.end(), obs15, obs15 + 15);
    W.idx_i.push_back(index_of(W.pose_index, W.poses, pose_i));
    W.idx_j.push_back(index_of(W.pose_index, W.poses, pose_j));
    W.idx_lm.push_back(index_of(W.lm_index, W.landmarks, invdepth));
    return true;
}

bool WindowFactorSet::upload(std::string *error) {
    n_factors_ = n_poses_ = n_lm_ = 0;
    std::vector<int32_t> fac_off{0}, lm_off{0};
    for (Window &W : windows_) {
        W.fac_begin = n_factors_, W.pose_begin = n_poses_, W.lm_begin = n_lm_;
        n_factors_ += W.size(), n_poses_ += (int) W.poses.size(), n_lm_ += (int) W.landmarks.size();
        fac_off.push_back(n_factors_), lm_off.push_back(n_lm_);
    }
    if (n_factors_ == 0) return true;
    // the windows' factors are written by the pool's threads straight into the context's pinned staging block (34 MB of observations at
    // 256 C2 windows: through a pageable vector and hipMemcpy they were most of this function's 13 ms)
    double *obs   = nullptr;
    int32_t *idx3 = nullptr;
    if (icg_reproj_stage_factors(ctx_, n_factors_, &obs, &idx3) != ICG_OK) {
        *error = icg_last_error(ctx_);
        return false;
    }
    int32_t *ii = idx3, *jj = idx3 + n_factors_, *ll = idx3 + 2 * (size_t) n_factors_;
    forEachWindow(windows_.size(), [&](size_t w) {
        const Window &W = windows_[w];
        for (int c = 0; c < 15; c++) { // (component-major: one contiguous destination run per component and window)
            double *dst = obs + (size_t) c * n_factors_ + (size_t) W.fac_begin;
            for (int k = 0; k < W.size(); k++) dst[k] = W.obs[(size_t) 15 * k + c];
        }
        for (int k = 0; k < W.size(); k++) {
            const size_t f = (size_t) W.fac_begin + (size_t) k;
            ii[f] = W.pose_begin + W.idx_i[(size_t) k], jj[f] = W.pose_begin + W.idx_j[(size_t) k], ll[f] = W.lm_begin + W.idx_lm[(size_t) k];
        }
    });
    if (icg_reproj_commit_factors(ctx_) != ICG_OK ||
        icg_reproj_set_windows(ctx_, (int) windows_.size(), fac_off.data(), lm_off.data()) != ICG_OK) {
        *error = icg_last_error(ctx_);
        return false;
    }
    return true;
}

void WindowFactorSet::gather(std::vector<double> &poses, std::vector<double> &ext, std::vector<double> &inv, std::vector<double> &td) {
    poses.resize(7 * (size_t) n_poses_), ext.assign(7 * windows_.size(), 0.0), inv.resize((size_t) n_lm_), td.assign(windows_.size(), 0.0);
    // (scattered reads through the callers' parameter pointers: spread over the pool like the other per-window phases)
    forEachWindow(windows_.size(), [&](size_t w) {
        const Window &W = windows_[w];
        for (size_t k = 0; k < W.poses.size(); k++) memcpy(&poses[7 * ((size_t) W.pose_begin + k)], W.poses[k], sizeof(double) * 7);
        for (size_t k = 0; k < W.landmarks.size(); k++) inv[(size_t) W.lm_begin + k] = *W.landmarks[k];
        if (W.ext)
            memcpy(&ext[7 * w], W.ext, sizeof(double) * 7);
        else
            ext[7 * w + 6] = 1.0;
        if (W.td) td[w] = *W.td;
    });
}

} // namespace icg
