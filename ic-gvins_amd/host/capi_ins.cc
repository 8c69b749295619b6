// C entry points of libicgvins_host.so: f4, MISC (misc_hip.h) driven through flat arrays: imu rows of 8, state rows of 23 (see
// include/icgvins_hip.h).
#include <string>
#include <vector>

#include "misc_hip.h"
#include "capi_util.h"

extern "C" {

int icgh_ins_mechanize(int n_streams, const int32_t *offsets, const double *imu, const double *cfg8, double *states23, double *traj23,
                       char *err, int errlen) {
    return guarded(err, errlen, [&] {
        TempCtx T(0);
        std::vector<std::vector<icg::IMU>> series((size_t) n_streams);
        std::vector<icg::IntegrationState> st((size_t) n_streams);
        std::vector<const std::vector<icg::IMU> *> sp;
        std::vector<icg::IntegrationState *> stp;
        for (int s = 0; s < n_streams; s++) {
            for (int r = offsets[s]; r < offsets[s + 1]; r++) series[(size_t) s].push_back(ins_imu(imu + 8 * (size_t) r));
            st[(size_t) s] = ins_state(states23 + 23 * (size_t) s);
            sp.push_back(&series[(size_t) s]);
            stp.push_back(&st[(size_t) s]);
        }
        std::vector<std::vector<icg::IntegrationState>> traj;
        std::string e;
        if (!icg::MISC::insMechanizationBatch(T.ctx, ins_config(cfg8), sp, stp, traj23 ? &traj : nullptr, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        for (int s = 0; s < n_streams; s++) {
            ins_put_state(st[(size_t) s], states23 + 23 * (size_t) s);
            if (traj23)
                for (size_t k = 0; k < traj[(size_t) s].size(); k++) ins_put_state(traj[(size_t) s][k], traj23 + 23 * ((size_t) offsets[s] + 1 + k));
        }
        return 0;
    });
}

// one (window, time) query per stream; windows are concatenated, stream s owns rows [win_offsets[s], win_offsets[s+1])
int icgh_ins_camera_pose(int n_streams, const int32_t *win_offsets, const double *imu, const double *states, const double *pose_b_c12,
                         const double *times, double *pose12_out, uint8_t *found_out, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        TempCtx T(0);
        std::vector<icg::InsWindow> w;
        std::vector<const icg::InsWindow *> wp;
        for (int s = 0; s < n_streams; s++)
            w.push_back(ins_window(win_offsets[s + 1] - win_offsets[s], imu + 8 * (size_t) win_offsets[s], states + 23 * (size_t) win_offsets[s]));
        for (auto &x : w) wp.push_back(&x);
        icg::Pose pbc;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) pbc.R(i, j) = pose_b_c12[3 * i + j];
            pbc.t[i] = pose_b_c12[9 + i];
        }
        std::vector<icg::Pose> poses;
        std::vector<uint8_t> found;
        std::string e;
        if (!icg::MISC::getCameraPoseFromInsWindowBatch(T.ctx, wp, pbc, std::vector<double>(times, times + n_streams), poses, found, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        for (int s = 0; s < n_streams; s++) {
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) pose12_out[12 * (size_t) s + 3 * i + j] = poses[(size_t) s].R(i, j);
                pose12_out[12 * (size_t) s + 9 + i] = poses[(size_t) s].t[i];
            }
            found_out[s] = found[(size_t) s];
        }
        return 0;
    });
}

// MISC::writeNavResult into <dir>/nav.txt, err.txt, traj.txt: `calls` consecutive calls with the same state (a row every 10th call)
int icgh_ins_write_nav_result(const double *cfg8, const double *origin3, const double *state23, double sodo, const char *dir, int calls) {
    icg::IntegrationConfiguration cfg = ins_config(cfg8);
    cfg.origin                        = icg::Vector3d(origin3[0], origin3[1], origin3[2]);
    icg::IntegrationState st          = ins_state(state23);
    st.sodo                           = sodo;
    std::string d(dir);
    auto nav = icg::FileSaver::create(d + "/nav.txt", 11), errf = icg::FileSaver::create(d + "/err.txt", 7), traj = icg::FileSaver::create(d + "/traj.txt", 8);
    if (!nav->isOpen() || !errf->isOpen() || !traj->isOpen()) return -1;
    for (int k = 0; k < calls; k++) icg::MISC::writeNavResult(cfg, st, nav, errf, traj);
    return 0;
}

long icgh_ins_window_index(int n_win, const double *imu, double time) {
    return (long) icg::MISC::getInsWindowIndex(ins_window(n_win, imu, nullptr), time);
}

// MISC::getImuSeriesFromTo: number of samples written, -1 on failure, -2 when cap is too small
int icgh_ins_imu_series(int n_win, const double *imu, double start, double end, int cap, double *series) {
    std::vector<icg::IMU> out;
    if (!icg::MISC::getImuSeriesFromTo(ins_window(n_win, imu, nullptr), start, end, out)) return -1;
    if ((int) out.size() > cap) return -2;
    for (size_t k = 0; k < out.size(); k++) ins_put_imu(out[k], series + 8 * k);
    return (int) out.size();
}

// MISC::redoInsMechanizationBatch: windows concatenated like icgh_ins_camera_pose; states updated in place, new_len[s] = the
// window length after the expired front entries were dropped (rows compacted to the front of each stream's slice)
int icgh_ins_redo(int n_streams, const double *cfg8, const double *updated23, int reserved, const int32_t *win_offsets, double *imu,
                  double *states, int32_t *new_len, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        TempCtx T(0);
        std::vector<icg::InsWindow> w;
        std::vector<icg::InsWindow *> wp;
        std::vector<icg::IntegrationState> upd;
        for (int s = 0; s < n_streams; s++) {
            w.push_back(ins_window(win_offsets[s + 1] - win_offsets[s], imu + 8 * (size_t) win_offsets[s], states + 23 * (size_t) win_offsets[s]));
            upd.push_back(ins_state(updated23 + 23 * (size_t) s));
        }
        for (auto &x : w) wp.push_back(&x);
        std::string e;
        if (!icg::MISC::redoInsMechanizationBatch(T.ctx, ins_config(cfg8), upd, (size_t) reserved, wp, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        for (int s = 0; s < n_streams; s++) {
            new_len[s] = (int32_t) w[(size_t) s].size();
            for (size_t k = 0; k < w[(size_t) s].size(); k++) {
                ins_put_imu(w[(size_t) s][k].first, imu + 8 * ((size_t) win_offsets[s] + k));
                ins_put_state(w[(size_t) s][k].second, states + 23 * ((size_t) win_offsets[s] + k));
            }
        }
        return 0;
    });
}

} // extern "C"
