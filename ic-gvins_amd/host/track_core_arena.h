// Host memory for one stream's I/O with the tracker core (track_core.h Io), for the executors that run the core's stage bodies on the
// host: TableTracker in core mode and the CPU stand-in of the device tracker's ABI.  Host only: track_core.h itself is compiled for the
// device and stays free of std::vector.  (The device executor's arena is a different thing: SoA across streams in HBM.)
#pragma once
#include <vector>

#include "track_core.h"

namespace tc {

struct HostArena { // this stream's segment of the primitives' work lists
    int32_t pre_slot{-1}, lk_count{0}, rs_count{0}, tri_count{0}, tri_n_tcw{0}, det_slot{-1}, det_mask_count{0}, det_count{0};
    double pre_hist{0};
    std::vector<int32_t> lk_prev_slot, lk_next_slot, tri_T0, tri_T1, det_quota;
    std::vector<P2f> lk_prev, lk_guess, lk_out, lk_undist, rs_p1, rs_p2, det_mask_pts, det_out;
    std::vector<uint8_t> lk_status, rs_mask;
    std::vector<double> tri_Tcw, tri_pc0, tri_pc1, tri_pw;

    void resize() {
        const size_t R = MAX_ROWS;
        lk_prev_slot.resize(R), lk_next_slot.resize(R), lk_prev.resize(R), lk_guess.resize(R), lk_out.resize(R), lk_undist.resize(R);
        lk_status.resize(R), rs_mask.resize(R), rs_p1.resize(R), rs_p2.resize(R), tri_T0.resize(R), tri_T1.resize(R);
        tri_Tcw.resize(12 * MAX_TCW), tri_pc0.resize(3 * R), tri_pc1.resize(3 * R), tri_pw.resize(3 * R);
        det_quota.resize(MAX_BLOCKS), det_mask_pts.resize(R), det_out.resize(R);
    }

    // lk_base: index of this stream's first point in the group's LK call
    Io io(int lk_base) {
        Io io;
        memset(&io, 0, sizeof io);
        io.pre_slot = &pre_slot, io.pre_hist = &pre_hist;
        io.lk_count = &lk_count, io.lk_prev_slot = lk_prev_slot.data(), io.lk_next_slot = lk_next_slot.data();
        io.lk_prev = lk_prev.data(), io.lk_guess = lk_guess.data(), io.lk_out = lk_out.data(), io.lk_undist = lk_undist.data();
        io.lk_status = lk_status.data(), io.lk_base = lk_base;
        io.rs_count = &rs_count, io.rs_p1 = rs_p1.data(), io.rs_p2 = rs_p2.data(), io.rs_mask = rs_mask.data();
        io.tri_count = &tri_count, io.tri_n_tcw = &tri_n_tcw, io.tri_T0 = tri_T0.data(), io.tri_T1 = tri_T1.data();
        io.tri_Tcw = tri_Tcw.data(), io.tri_pc0 = tri_pc0.data(), io.tri_pc1 = tri_pc1.data(), io.tri_pw = tri_pw.data();
        io.det_slot = &det_slot, io.det_quota = det_quota.data(), io.det_mask_count = &det_mask_count;
        io.det_mask_pts = det_mask_pts.data(), io.det_count = &det_count, io.det_out = det_out.data();
        return io;
    }
};

} // namespace tc
