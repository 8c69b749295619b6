// The windows the marginalization entries (capi_marg_resident.cc, capi_marg_prior.cc) hand to a MarginalizationBatch, shared like
// capi_windows.h (internal linkage, included by capi_*.cc and nothing else): one Case per window whatever built it, the visual windows of
// capi_windows.h as cases, and those windows one keyframe later with the first marginalization's prior among their host factors.
#pragma once
#include <algorithm>
#include <memory>

#include "capi_windows.h"

namespace {

using icg::vector;

// One window to marginalize, whatever built it: the info with every factor added, the addresses of its parameter ids, and its
// reprojection factors with their five blocks for MarginalizationBatch::addReprojectionFactor / ReprojectionBatch::add.
struct Case {
    std::shared_ptr<icg::MarginalizationInfo> info;
    std::unordered_map<long, long> ids;
    std::unordered_map<long, double *> address;
    struct Reproj {
        icg::ReprojectionFactor *factor;
        double *blocks[5];
    };
    vector<Reproj> reproj;
    vector<std::shared_ptr<icg::ReprojectionFactor>> owned;
    vector<std::shared_ptr<void>> keep; // whatever else has to live as long as the window (the family's own parameter arrays)
    template <class Add>
    void addReprojections(Add &&add) {
        for (Reproj &R : reproj) add(R.factor, R.blocks[0], R.blocks[1], R.blocks[2], R.blocks[3], R.blocks[4]);
    }
};

// family 0: the jittered visual windows of icgh_backend_marginalize_batch
std::unique_ptr<Case> visual_case(const MargArgs &a, MargWindow &W) {
    std::unique_ptr<Case> c(new Case);
    c->info = W.info, c->ids = W.ids, c->address = W.address;
    for (int k = 0; k < a.n; k++)
        c->reproj.push_back({W.factors[(size_t) k].get(),
                             {&W.P[7 * (size_t) a.idx_i[k]], &W.P[7 * (size_t) a.idx_j[k]], W.E.data(), &W.D[(size_t) a.idx_lm[k]], &W.TD}});
    return c;
}
vector<std::unique_ptr<Case>> visual_cases(const MargArgs &a, vector<std::unique_ptr<MargWindow>> &wins) {
    vector<std::unique_ptr<Case>> out;
    for (auto &W : wins) out.push_back(visual_case(a, *W));
    return out;
}

// family 2: the windows of family 0 one keyframe later.  Generation 1 (`wins`, marginalized by the caller) left a prior on the retained
// blocks; now keyframe 1 leaves: the MarginalizationFactor of generation 1 is a host factor over all of its blocks, and the reprojection
// factors are the ones anchored in keyframe 1 (the second factor table, indices into the same poses and inverse depths).  The positions of
// the retained keyframes are moved by `jitter` first, so that the prior is evaluated away from its linearization point.
struct SecondTable {
    int n2;
    const double *obs2_soa;
    const int32_t *idx2_i, *idx2_j, *idx2_lm;
};
// what one second-generation window may carry beyond that (capi_marg_prior.cc's mixed batch)
struct SecondExtras {
    bool robust_prior  = false; // the prior gets a Huber loss: it is no plain prior any more
    bool lm_host_factor = false; // a host factor on an inverse depth that leaves: the window is not planned (dense path)
    bool weak_landmark = false; // one more inverse depth seen by a single factor of negligible weight: h_ll fails the first guard
};
std::unique_ptr<Case> second_generation_case(const MargArgs &a, MargWindow &W, const SecondTable &t, double jitter, Uniform &rnd,
                                             const SecondExtras &extras = SecondExtras()) {
    using namespace icg;
    auto loss = a.huber_delta > 0 ? std::make_shared<HuberLossHip>(a.huber_delta) : nullptr;
    std::unique_ptr<Case> c(new Case);
    c->ids = W.ids, c->address = W.address;
    const vector<double *> blocks = W.info->getParamterBlocks(W.address);
    auto prior                    = std::make_shared<MarginalizationFactor>(W.info);
    for (int k = 1; k < a.n_poses; k++)
        for (int x = 0; x < 3; x++) W.P[7 * (size_t) k + x] += jitter * rnd();
    c->info = std::make_shared<MarginalizationInfo>();
    vector<int> drop;
    for (size_t k = 0; k < blocks.size(); k++)
        if (blocks[k] == &W.P[7]) drop.push_back((int) k);
    std::shared_ptr<double> weak;
    if (extras.weak_landmark && t.n2 > 0) {
        weak = std::make_shared<double>(W.D[(size_t) t.idx2_lm[0]]);
        c->keep.push_back(weak);
        c->ids[reinterpret_cast<long>(weak.get())] = 100000 + a.n_lm, c->address[100000 + a.n_lm] = weak.get();
    }
    c->info->updateParamtersIds(c->ids);
    c->info->addResidualBlockInfo(std::make_shared<ResidualBlockInfo>(
        prior, extras.robust_prior ? std::make_shared<HuberLossHip>(a.huber_delta > 0 ? a.huber_delta : 1.0) : nullptr, blocks, drop));
    auto add = [&](std::shared_ptr<ReprojectionFactor> f, double *pi, double *pj, double *lm) {
        c->owned.push_back(std::move(f));
        c->info->addResidualBlockInfo(
            std::make_shared<ResidualBlockInfo>(c->owned.back(), loss, vector<double *>{pi, pj, W.E.data(), lm, &W.TD}, vector<int>{0, 3}));
        c->reproj.push_back({c->owned.back().get(), {pi, pj, W.E.data(), lm, &W.TD}});
    };
    for (int k = 0; k < t.n2; k++)
        add(reproj_factor_from_soa(t.obs2_soa, t.n2, k), &W.P[7 * (size_t) t.idx2_i[k]], &W.P[7 * (size_t) t.idx2_j[k]], &W.D[(size_t) t.idx2_lm[k]]);
    if (weak) { // factor 0 of the table once more, on the extra inverse depth, with a standard deviation of 1e6
        auto o = [&](int col) { return t.obs2_soa[(size_t) col * t.n2]; };
        add(std::make_shared<ReprojectionFactor>(Vector3d(o(0), o(1), o(2)), Vector3d(o(3), o(4), o(5)), Vector3d(o(6), o(7), o(8)), Vector3d(o(9), o(10), o(11)),
                                                 o(12), o(13), 1e6),
            &W.P[7 * (size_t) t.idx2_i[0]], &W.P[7 * (size_t) t.idx2_j[0]], weak.get());
    }
    if (extras.lm_host_factor && t.n2 > 0) {
        double *lm = &W.D[(size_t) t.idx2_lm[0]];
        c->info->addResidualBlockInfo(std::make_shared<ResidualBlockInfo>(std::make_shared<ScalarPriorFactor>(*lm * 1.01, 0.5 * a.prior_weight), nullptr,
                                                                          vector<double *>{lm}, vector<int>{0}));
    }
    return c;
}
vector<std::unique_ptr<Case>> second_generation(const MargArgs &a, vector<std::unique_ptr<MargWindow>> &wins, int n2, const double *obs2_soa, const int32_t *idx2_i,
                                                const int32_t *idx2_j, const int32_t *idx2_lm, double jitter) {
    vector<std::unique_ptr<Case>> out;
    Uniform rnd{kJitterSeed ^ 0x5DEECE66Dull};
    const SecondTable t{n2, obs2_soa, idx2_i, idx2_j, idx2_lm};
    for (auto &W : wins) out.push_back(second_generation_case(a, *W, t, jitter, rnd));
    return out;
}

// What the entries return of a marginalized batch.  Per window w: ok_out[w], r_out[w] (0 when not ok), tag_slot[w] (its index in the kept
// linearization, -1: untagged); Hp, J0 (r x r) and bp, e0 (r) of the good windows, concatenated in window order.  Then `mb` is cleared, and
// a MarginalizationFactor per good window goes into a MarginalizationPriorSet set from their views on a SECOND context and evaluated at
// x = x0 + perturb * u (u from `seed`): residuals (sum r).  *tagged: tagged windows; *handed_off: windows the set took from the kept
// linearization.  0, or -3 with the set's message.
int marg_case_outputs(vector<std::unique_ptr<Case>> &cases, const vector<char> &ok, icg::MarginalizationBatch &mb, uint64_t seed, double perturb, uint8_t *ok_out,
                      int32_t *r_out, int32_t *tag_slot, double *Hp, double *bp, double *J0, double *e0, double *residuals, int32_t *tagged, int32_t *handed_off,
                      char *err, int errlen) {
    using namespace icg;
    vector<std::shared_ptr<MarginalizationFactor>> priors;
    size_t at = 0, at2 = 0;
    for (size_t w = 0; w < cases.size(); w++) {
        ok_out[w] = ok[w] ? 1 : 0;
        if (!ok[w]) continue;
        Case &c                      = *cases[w];
        const MarginalizationInfo &I = *c.info;
        const size_t r               = (size_t) I.remainedSize();
        r_out[w]                     = (int32_t) r;
        memcpy(Hp + at2, I.Hp().data(), sizeof(double) * r * r), memcpy(J0 + at2, I.linearizedJacobians().data(), sizeof(double) * r * r);
        memcpy(bp + at, I.bp().data(), sizeof(double) * r), memcpy(e0 + at, I.linearizedResiduals().data(), sizeof(double) * r);
        at += r, at2 += r * r;
        if (I.keptId() != 0) tag_slot[w] = I.keptSlot(), (*tagged)++;
        (void) c.info->getParamterBlocks(c.address); // (fills the remained-block lists the factor copies)
        priors.push_back(std::make_shared<MarginalizationFactor>(c.info));
    }
    mb.clear();
    if (priors.empty()) return 0;
    TempCtx T(0);
    MarginalizationPriorSet set;
    vector<MargPriorView> views;
    for (auto &f : priors) views.push_back(f->margPriorView());
    std::string e;
    if (!set.set(T.ctx, views, &e)) {
        set_err(err, errlen, e.c_str());
        return -3;
    }
    *handed_off = set.handedOff();
    Uniform rnd = point_stream(seed);
    vector<vector<double>> xs(views.size());
    vector<vector<const double *>> params(views.size());
    vector<const double *const *> plist(views.size());
    for (size_t p = 0; p < views.size(); p++) {
        const MargPriorView &v = views[p];
        for (int b = 0; b < v.n_blocks; b++)
            for (int k = 0; k < v.size[b]; k++) xs[p].push_back(v.x0[b][k] + perturb * rnd());
        size_t off = 0;
        for (int b = 0; b < v.n_blocks; b++) params[p].push_back(xs[p].data() + off), off += (size_t) v.size[b];
        plist[p] = params[p].data();
    }
    if (!set.evaluate(plist, residuals, nullptr, nullptr, nullptr, &e)) {
        set_err(err, errlen, e.c_str());
        return -3;
    }
    return 0;
}

} // namespace
