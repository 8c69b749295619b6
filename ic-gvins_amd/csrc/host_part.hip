// f1: the host-factor part of every window's reduced camera system, built where icg_reproj_solve_windows reads it.
//
// A window's host-evaluated factors (preintegration, the marginalization prior, pose / mix / GNSS priors) arrive as blocks: nr residuals,
// a dense row-major nr x nf Jacobian of the factor's free local columns and the nf columns they occupy in the window's system.  The packed
// lower triangle of sum_blocks J^T J goes into the window's slot of d_red_H, -J^T r and diag(J^T J) go back to the host; the values are the
// ones solver_detail::hostFactors forms (host/solver_detail.h), bit for bit: every block value is a sum over the residual index in ascending
// order from +0.0 (one multiply, one add per term: this file is compiled with -ffp-contract=off like the rest), and every cell receives the
// block values in block order.  One thread owns a cell through all blocks, so nothing is added atomically and a window's bits do not depend
// on the batch it is built in.  The Jacobians stay on the device (icg_hp_kept): a block whose Jacobian did not change crosses the link as
// its residuals only.  A block that is a marginalization prior resident on the device (marg.hip) crosses it not at all
// (icg_reproj_host_parts_build_prior): k_host_part_prior copies its residuals of the last resident evaluation and the free columns of its J0
// to the places k_host_part reads.  The same kernel serves a block that is a preintegration factor of the resident P2 set (preint.hip,
// icg_reproj_host_parts_build_preint): its source matrix is the factor's whitened 15 x 32 Jacobian, its row stride 32; and a factor of the
// resident odometer P2 set (preint_odo.hip, icg_reproj_host_parts_build_preint_odo): 19 x 34, row stride 34; and a member of the resident nav set
// (nav.hip, icg_reproj_host_parts_build_nav): nr x width, row stride the member's block width.  On the host side a family of resident blocks is
// one line of hp_families (its rules, its gather code, its entry and the words of its messages); validation and staging loop over that table,
// and the five exported entries hand hp_build the tables of the families they have.
#include <array>

#include "reproj_internal.h"

#define HP_THREADS 256
#define HP_CPT 16     // cells of the packed triangle per thread: a workgroup owns HP_THREADS * HP_CPT consecutive cells of one window
#define HP_STAGE 4096 // doubles of a block's Jacobian rows staged in LDS per pass (32 KB)
#define HP_MAX_KC 64  // rows per pass at the most
#define HP_MAX_P 512  // columns of a reduced system at the most: what the entry admits (nf <= Pw <= P) and the column tables in LDS hold
static_assert(HP_MAX_P <= 2 * HP_THREADS, "the first workgroup of a window owns s and diag in two columns per thread");
static_assert(HP_STAGE / HP_MAX_P >= 1, "a staging pass holds at least one row of the widest block");

struct hp_win {
    int32_t w, Pw, blk_begin, blk_end, slot, pad; // blocks [blk_begin, blk_end) of the call's block list; slot: index among the rebuilt windows
    int64_t H_off, out_off;                       // the window's slot in d_red_H and its triangle in part_out
};
struct hp_blk {
    int64_t J_off; // into the kept Jacobians
    int32_t r_off, cols_off, nr, nf;
};
struct hp_copy {
    int64_t src, dst, n;
};
#define HP_PRIOR_ROWS 16 // rows of a resident block per workgroup of k_host_part_prior
// A block whose residual and Jacobian are resident on the device: a marginalization prior (J = its J0, row stride r) or a preintegration factor
// of the resident P2 set (J = its whitened 15 x 32 Jacobian, row stride 32) or of the resident odometer P2 set (19 x 34, row stride 34).
struct hp_prior {
    const double *J, *res;        // the block's source matrix and residuals on the device
    int64_t Jd_off;               // the block's place among the kept Jacobians
    int32_t stride, r_off, pc_off; // row stride of J; the block's place in the staged r; its columns of J in the staged column list
    int32_t nr, nf, fill;         // fill != 0: the kept Jacobian is gathered from J (ICG_HP_JAC_FROM_PRIOR / _PREINT / _PREINT_ODO)
};

// the shipped Jacobians move from the staging arena to their places among the kept ones: one workgroup per shipped block
__global__ __launch_bounds__(HP_THREADS) void k_host_part_keep(const hp_copy *cp, const double *src, double *dst) {
    const hp_copy c = cp[blockIdx.x];
    for (int64_t e = threadIdx.x; e < c.n; e += HP_THREADS) dst[c.dst + e] = src[c.src + e];
}

// grid (ceil(max cells / (HP_THREADS * HP_CPT)), rebuilt windows).  Thread t of workgroup g owns the cells g * 4096 + t + 256 i (i < 16) of the
// packed triangle in registers; the window's first workgroup also owns s and diag (columns t and t + 256: P <= 512).  Per block: the column ->
// local index map of the block in LDS, then its Jacobian rows in passes of at most HP_STAGE doubles, each cell adding J[k][x] J[k][y] for
// the rows of the pass in ascending k.
__global__ __launch_bounds__(HP_THREADS) void k_host_part(const hp_win *wins, const hp_blk *blks, const int32_t *cols, const double *J, const double *r, int P,
                                                          double *H, double *s_out, double *diag_out, double *part_out) {
    __shared__ double Js[HP_STAGE];
    __shared__ double rs[HP_MAX_KC];
    __shared__ int16_t map[HP_MAX_P];
    const hp_win W    = wins[blockIdx.y];
    const int n_cells = (W.Pw * (W.Pw + 1)) >> 1, base = blockIdx.x * (HP_THREADS * HP_CPT);
    if (base >= n_cells) return; // (a narrower window than the widest of the call: uniform over the workgroup)
    const int t      = threadIdx.x;
    const bool first = blockIdx.x == 0;
    int ab[HP_CPT]; // row | column << 16 of cell i, -1 beyond the triangle
    double acc[HP_CPT];
#pragma unroll
    for (int i = 0; i < HP_CPT; i++) {
        const int c = base + t + HP_THREADS * i;
        int a       = (int) ((sqrtf(8.0f * (float) c + 1.0f) - 1.0f) * 0.5f);
        while ((a + 1) * (a + 2) / 2 <= c) a++;
        while (a * (a + 1) / 2 > c) a--;
        ab[i]  = c < n_cells ? (a | (c - a * (a + 1) / 2) << 16) : -1;
        acc[i] = 0.0;
    }
    double s[2] = {0.0, 0.0}, dg[2] = {0.0, 0.0};
    for (int b = W.blk_begin; b < W.blk_end; b++) {
        const hp_blk B = blks[b];
        const int nf   = B.nf;
        __syncthreads(); // (the previous block's map and rows have been read)
        for (int c = t; c < W.Pw; c += HP_THREADS) map[c] = -1;
        __syncthreads();
        for (int x = t; x < nf; x += HP_THREADS) map[cols[B.cols_off + x]] = (int16_t) x;
        __syncthreads();
        int xy[HP_CPT]; // local indices x | y << 16 of the cells the block holds, -1 for the others
        double T[HP_CPT];
        bool any = false;
#pragma unroll
        for (int i = 0; i < HP_CPT; i++) {
            const int x = ab[i] >= 0 ? map[ab[i] & 0xffff] : -1, y = ab[i] >= 0 ? map[ab[i] >> 16] : -1;
            xy[i]       = x >= 0 && y >= 0 ? (x | y << 16) : -1;
            any |= xy[i] >= 0;
            T[i] = 0.0;
        }
        int sx[2];
        double g[2] = {0.0, 0.0}, d[2] = {0.0, 0.0};
#pragma unroll
        for (int k = 0; k < 2; k++) sx[k] = first && t + HP_THREADS * k < W.Pw ? map[t + HP_THREADS * k] : -1;
        const int KC    = min(HP_MAX_KC, HP_STAGE / nf); // nf <= 512: at least 8 rows
        const double *Jb = J + B.J_off;
        for (int k0 = 0; k0 < B.nr; k0 += KC) {
            const int kc = min(KC, B.nr - k0);
            __syncthreads();
            for (int e = t; e < kc * nf; e += HP_THREADS) Js[e] = Jb[(size_t) k0 * nf + e];
            if (t < kc) rs[t] = r[B.r_off + k0 + t];
            __syncthreads();
            if (any) {
                for (int kk = 0; kk < kc; kk++) {
                    const double *row = Js + kk * nf;
#pragma unroll
                    for (int i = 0; i < HP_CPT; i++)
                        if (xy[i] >= 0) T[i] += row[xy[i] & 0xffff] * row[xy[i] >> 16];
                }
            }
#pragma unroll
            for (int k = 0; k < 2; k++)
                if (sx[k] >= 0)
                    for (int kk = 0; kk < kc; kk++) {
                        const double jx = Js[kk * nf + sx[k]];
                        g[k] += jx * rs[kk];
                        d[k] += jx * jx;
                    }
        }
#pragma unroll
        for (int i = 0; i < HP_CPT; i++)
            if (xy[i] >= 0) acc[i] += T[i];
#pragma unroll
        for (int k = 0; k < 2; k++)
            if (sx[k] >= 0) s[k] -= g[k], dg[k] += d[k];
    }
#pragma unroll
    for (int i = 0; i < HP_CPT; i++) {
        const int c = base + t + HP_THREADS * i;
        if (c >= n_cells) continue;
        H[W.H_off + c] = acc[i];
        if (part_out) part_out[W.out_off + c] = acc[i];
    }
    if (first) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int c = t + HP_THREADS * k;
            if (c < P) s_out[(size_t) W.slot * P + c] = s[k], diag_out[(size_t) W.slot * P + c] = dg[k]; // (zeros from Pw up to P)
        }
    }
}

// A block that is resident on the device (a marginalization prior of icg_marg_prior_set, a factor of icg_preint_set or icg_preint_odo_set), for the row tile
// blockIdx.x of the resident block blockIdx.y: the kept Jacobian is gathered from the block's row-major source matrix where the block asks for it
// (Jd[k][y] = J[k][pc[y]]: the elements of a tile are consecutive in Jd, so the writes are contiguous along y and across the rows of the tile),
// and the residuals of the last resident evaluation are copied to the block's place in the staged r.  A plain copy without atomics, ahead of
// k_host_part.
__global__ __launch_bounds__(HP_THREADS) void k_host_part_prior(const hp_prior *pr, const int32_t *pcols, double *Jd, double *r) {
    __shared__ int32_t pc[HP_MAX_P]; // (nf <= HP_MAX_P: the entry's capacity check)
    const hp_prior B = pr[blockIdx.y];
    const int k0 = blockIdx.x * HP_PRIOR_ROWS, t = threadIdx.x;
    if (k0 >= B.nr) return; // (a shorter block than the longest of the call: uniform over the workgroup)
    const int kc = min(HP_PRIOR_ROWS, B.nr - k0);
    if (t < kc) r[B.r_off + k0 + t] = B.res[k0 + t];
    if (!B.fill) return;
    for (int y = t; y < B.nf; y += HP_THREADS) pc[y] = pcols[B.pc_off + y];
    __syncthreads();
    const double *src = B.J + (size_t) k0 * B.stride;
    double *dst       = Jd + B.Jd_off + (size_t) k0 * B.nf;
    for (int e = t; e < kc * B.nf; e += HP_THREADS) {
        const int k = e / B.nf, y = e - k * B.nf;
        dst[e]      = src[(size_t) k * B.stride + pc[y]];
    }
}

// ---- the entry, in stages: hp_validate (a plan; nothing is changed) -> hp_place_kept -> hp_stage -> hp_launch (launch and commit) -------------------------
struct hp_args { // the arguments of a call as the stages read them; me: the entry a message names, W: the windows of the partition
    const char *me;
    int P, W;
    const int32_t *Pw, *blk_off, *nr, *nf, *cols;
    const uint8_t *rebuild;
    const int64_t *jac_off;
    const double *J, *r;
    double *host_s, *host_diag, *part_out;
};
// A family of device-resident blocks: what hp_families (below the rules) says of it once, and what a call brings for it.  Its rules: may member idx of the
// family's resident set be block p of window w, B.nr residuals whose kept Jacobian holds the columns pc[0 .. B.nf) of the member's source matrix (B.fill:
// gathered in this call)?  They fill in the member's source, residuals and row stride.
typedef int hp_rules(icg_ctx *ctx, const char *me, int w, int p, int idx, const int32_t *pc, hp_prior &B);
struct hp_family {
    hp_rules *rules;
    int64_t gather;     // the jac_off that asks for the kept Jacobian to be gathered from the member's source
    const char *entry;  // the narrowest entry that takes the family's tables: a call's messages name the widest family whose table it was given
    const char *member; // article and noun, as in "both a prior (0) and a navigation factor (1)"
    // a block outside the family that asks for `gather` is refused as "<jac_name> for a block that is no <no_member>"; jac_name NULL: as "jac_off = <value>",
    // and so it is with named_with_of in a call without the family's table (an older entry reports the value, as it always did)
    const char *jac_name, *no_member;
    bool named_with_of;
    const int32_t *of, *cols; // the call's: per block its member of the set (< 0: none; NULL: no block of the call); the members' columns, block after block
    size_t at;                // walks cols over the family's blocks of ALL windows (a window that is not rebuilt still places the others')
};

// What every family asks first: is its set (n members, results o, made resident by <stem>_set and evaluated by <stem>_evaluate_resident) resident and
// evaluated, with Jacobians when the block gathers them, and is member idx inside it?  what: the set's noun; member, set: the nouns of the second
// refusal; pending: a refusal of the family's own that stands between the two (NULL: none).
static int hp_require(icg_ctx *ctx, const char *me, int w, int p, const icg_resident_results &o, int n, bool need_jac, int idx, const char *what, const char *stem,
                      const char *member, const char *set, const char *pending = nullptr) {
    if (n <= 0 || !o.res_valid || (need_jac && !o.jac_valid))
        return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: no %s set is resident and evaluated%s (%s_set, then %s_evaluate_resident)", me, w, p, what,
                        need_jac ? " with Jacobians" : "", stem, stem);
    if (pending) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %s", me, w, p, pending);
    if (idx >= n) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %s %d outside the resident %sset of %d", me, w, p, member, idx, set, n);
    return ICG_OK;
}

static int hp_rules_prior(icg_ctx *ctx, const char *me, int w, int p, int pp, const int32_t *pc, hp_prior &B) {
    const icg_marg_set &ms = ctx->marg;
    if (!pc) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: a prior block without prior_cols", me, w, p);
    if (int rc = hp_require(ctx, me, w, p, ms.out, ms.n, false, pp, "prior", "icg_marg_prior", "prior", "")) return rc; // (J0 is the set's own: no Jacobians to ask for)
    const int pr = ms.h_r[(size_t) pp];
    if (B.nr != pr) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %d residuals, prior %d has %d", me, w, p, B.nr, pp, pr);
    for (int x = 0; x < B.nf; x++)
        if (pc[x] < 0 || pc[x] >= pr) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: prior column %d outside the prior (%d)", me, w, p, pc[x], pr);
    B.J = ms.d_J + ms.h_j_off[(size_t) pp], B.res = ms.out.d_res + ms.h_e_off[(size_t) pp], B.stride = pr; // (J0 is r x r)
    return ICG_OK;
}

static int hp_rules_preint(icg_ctx *ctx, const char *me, int w, int p, int fp, const int32_t *pc, hp_prior &B) {
    const icg_preint_resident &ps = ctx->preint;
    if (!pc) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: a preintegration block without preint_cols", me, w, p);
    if (int rc = hp_require(ctx, me, w, p, ps.out, ps.n, B.fill, fp, "preintegration", "icg_preint", "factor", "")) return rc;
    if (B.nr != 15) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %d residuals, a preintegration factor has 15", me, w, p, B.nr);
    for (int x = 0; x < B.nf; x++)
        if (pc[x] < 0 || pc[x] >= 32 || pc[x] == 6 || pc[x] == 22)
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: preintegration column %d (0 .. 31 without 6 and 22)", me, w, p, pc[x]);
    B.J = ps.out.d_jac ? ps.out.d_jac + 480 * (size_t) fp : nullptr, B.res = ps.out.d_res + 15 * (size_t) fp, B.stride = 32; // (the whitened 15 x 32 Jacobian)
    return ICG_OK;
}

static int hp_rules_preint_odo(icg_ctx *ctx, const char *me, int w, int p, int fp, const int32_t *pc, hp_prior &B) {
    const icg_preint_resident &ps = ctx->preint_odo;
    if (!pc) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: an odometer preintegration block without preint_odo_cols", me, w, p);
    if (int rc = hp_require(ctx, me, w, p, ps.out, ps.n, B.fill, fp, "odometer preintegration", "icg_preint_odo", "factor", "odometer ")) return rc;
    if (B.nr != 19) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %d residuals, an odometer preintegration factor has 19", me, w, p, B.nr);
    for (int x = 0; x < B.nf; x++)
        if (pc[x] < 0 || pc[x] >= 34 || pc[x] == 6 || pc[x] == 23)
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: odometer preintegration column %d (0 .. 33 without 6 and 23)", me, w, p, pc[x]);
    B.J = ps.out.d_jac ? ps.out.d_jac + 646 * (size_t) fp : nullptr, B.res = ps.out.d_res + 19 * (size_t) fp, B.stride = 34; // (the whitened 19 x 34 Jacobian)
    return ICG_OK;
}

static int hp_rules_nav(icg_ctx *ctx, const char *me, int w, int p, int fp, const int32_t *pc, hp_prior &B) {
    const icg_nav_resident &ns = ctx->nav;
    if (!pc) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: a navigation block without nav_cols", me, w, p);
    const char *uncorrected = B.fill && ns.any_robust && !ns.corrected
                                  ? "the nav set has robustified members and its last evaluation is not corrected (icg_nav_correct_resident first)"
                                  : nullptr;
    if (int rc = hp_require(ctx, me, w, p, ns.out, ns.n, B.fill, fp, "nav", "icg_nav", "member", "nav ", uncorrected)) return rc;
    const int kind = ns.h_kind[(size_t) fp], width = icg_nav_width(kind);
    if (B.nr != icg_nav_nr(kind))
        return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %d residuals, nav member %d (kind %d) has %d", me, w, p, B.nr, fp, kind, icg_nav_nr(kind));
    for (int x = 0; x < B.nf; x++)
        if (pc[x] < 0 || pc[x] >= width || (width == 7 && pc[x] == 6))
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: navigation column %d (0 .. %d%s)", me, w, p, pc[x], width - 1, width == 7 ? " without 6" : "");
    B.J = ns.out.d_jac ? ns.out.d_jac + ns.h_j_off[(size_t) fp] : nullptr, B.res = ns.out.d_res + ns.h_r_off[(size_t) fp], B.stride = width; // (row-major nr x width)
    return ICG_OK;
}

// The families, narrowest entry first: a new one is a line here, its rules above and its entry at the foot of the file.
static const hp_family hp_families[] = {
    {hp_rules_prior, ICG_HP_JAC_FROM_PRIOR, "icg_reproj_host_parts_build_prior", "a prior", nullptr, nullptr, false},
    {hp_rules_preint, ICG_HP_JAC_FROM_PREINT, "icg_reproj_host_parts_build_preint", "a preintegration factor", "ICG_HP_JAC_FROM_PREINT", "preintegration factor", false},
    {hp_rules_preint_odo, ICG_HP_JAC_FROM_PREINT_ODO, "icg_reproj_host_parts_build_preint_odo", "an odometer preintegration factor", "ICG_HP_JAC_FROM_PREINT_ODO",
     "odometer preintegration factor", false},
    {hp_rules_nav, ICG_HP_JAC_FROM_NAV, "icg_reproj_host_parts_build_nav", "a navigation factor", "ICG_HP_JAC_FROM_NAV", "navigation factor", true}};
constexpr int HP_FAMILIES = (int) (sizeof(hp_families) / sizeof(hp_families[0]));
struct hp_plan { // what validation leaves for the stages behind it
    bool drop_all, have_kept;
    std::vector<int32_t> r_off, c_off; // every block's place in the staged r and cols
    std::vector<hp_prior> res;                // the resident blocks of the rebuilt windows ...
    std::vector<std::array<int, 3>> res_at;   // ... their (window, position in the window's block list, family)
    std::vector<int32_t> res_cols; // the staged column list their pc_off counts in: prior_cols | preint_cols | preint_odo_cols | nav_cols of all windows (each may be absent)
    size_t n_res_cols = 0, ship_doubles = 0, out_cells = 0; // (n_res_cols: what the families' cursors walked)
    int n_rebuilt = 0, max_cells = 0, max_prior_nr = 0;
};

// block b of the rebuilt window w behind its shape and capacity: nf > Pw, columns, the rules of its family (idx[f] >= 0: member idx[f], columns from c0[f]), jac_off
static int hp_validate_block(icg_ctx *ctx, const hp_args &a, const hp_family (&F)[HP_FAMILIES], const int (&idx)[HP_FAMILIES], const size_t (&c0)[HP_FAMILIES], int w, int b,
                             const std::vector<icg_hp_block> *kept, std::vector<int32_t> &seen, bool &any_keep, hp_plan &plan) {
    const char *me = a.me;
    const int p = b - a.blk_off[w], nr = a.nr[b], nf = a.nf[b], Pw = a.Pw[w];
    if (nf > Pw) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %d columns in a system of %d", me, w, p, nf, Pw);
    for (int x = 0; x < nf; x++) {
        const int c = a.cols[(size_t) plan.c_off[(size_t) b] + x];
        if (c < 0 || c >= Pw) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: column %d outside the system (%d)", me, w, p, c, Pw);
        if (seen[(size_t) c] == b) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: column %d twice", me, w, p, c);
        seen[(size_t) c] = b;
    }
    int fam = -1; // the family the block is resident in
    for (int f = 0; f < HP_FAMILIES; f++) {
        if (idx[f] < 0) continue;
        if (fam >= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: both %s (%d) and %s (%d)", me, w, p, F[fam].member, idx[fam], F[f].member, idx[f]);
        fam = f;
        hp_prior B{nullptr, nullptr, 0 /* its place among the kept Jacobians: hp_stage */, 0, plan.r_off[(size_t) b], (int32_t) c0[f], nr, nf, a.jac_off[b] == F[f].gather ? 1 : 0};
        if (int rc = F[f].rules(ctx, me, w, p, idx[f], F[f].cols ? F[f].cols + c0[f] : nullptr, B)) return rc;
        plan.res.push_back(B), plan.res_at.push_back({w, p, f});
        plan.max_prior_nr = std::max(plan.max_prior_nr, nr);
    }
    if (a.jac_off[b] >= 0) {
        if (!a.J) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: a Jacobian offset without J", me, w, p);
        plan.ship_doubles += (size_t) nr * nf;
    } else if (fam >= 0 && a.jac_off[b] == F[fam].gather) {
        // gathered on the device: from the prior's J0, from the factor's resident Jacobian
    } else if (a.jac_off[b] == -1) {
        any_keep = true;
        if (!kept || (size_t) p >= kept->size()) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: no kept Jacobian", me, w, p);
        const icg_hp_block &k = (*kept)[(size_t) p];
        if (k.nr != nr || k.nf != nf)
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: the kept Jacobian is %d x %d, not %d x %d", me, w, p, k.nr, k.nf, nr, nf);
    } else {
        for (const hp_family &G : F) // another family's gather code
            if (a.jac_off[b] == G.gather && G.jac_name && (G.of || !G.named_with_of))
                return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %s for a block that is no %s", me, w, p, G.jac_name, G.no_member);
        return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: jac_off = %lld", me, w, p, (long long) a.jac_off[b]);
    }
    return ICG_OK;
}

// Stage 1.  Nothing is changed before validation is through: no field of ctx is written here and nothing is allocated on the device.
static int hp_validate(icg_ctx *ctx, const hp_args &a, hp_family (&F)[HP_FAMILIES], hp_plan &plan) {
    const char *me = a.me;
    const int P = a.P, W = a.W;
    if (W <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: no window partition: call icg_reproj_set_windows first", me);
    if (P <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: P = %d", me, P);
    if (P > HP_MAX_P) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: reduced systems of more than %d camera columns are not supported (%d)", me, HP_MAX_P, P);
    if (W > 65535) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: %d windows in one call (at most 65535)", me, W);
    if (ctx->red_W != 0 && ctx->red_P != P) return icg_fail(ctx, ICG_ERR_INVALID, "%s: P = %d, the resident reduced systems have %d columns", me, P, ctx->red_P);
    if (!a.Pw || !a.rebuild || !a.blk_off || !a.host_s || !a.host_diag) return icg_fail(ctx, ICG_ERR_INVALID, "%s: NULL argument", me);
    if (a.blk_off[0] != 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window 0: blk_off[0] = %d", me, a.blk_off[0]);
    for (int w = 0; w < W; w++)
        if (a.blk_off[w + 1] < a.blk_off[w])
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d: blk_off decreases (%d after %d)", me, w, a.blk_off[w + 1], a.blk_off[w]);
    const int nb = a.blk_off[W];
    if (nb > 0 && (!a.nr || !a.nf || !a.cols || !a.jac_off || !a.r)) return icg_fail(ctx, ICG_ERR_INVALID, "%s: NULL argument", me);
    // the slots of d_red_H follow the P of the resident reduced systems, or of the last call here while there are none: host parts (and
    // kept Jacobians) of another shape, or of a buffer that is about to be replaced, are dropped before this call's are built
    const size_t H_bytes = sizeof(double) * (size_t) W * ((size_t) P * (P + 1) / 2);
    plan.drop_all        = ctx->red_H_cols.size() != (size_t) W || (ctx->red_W == 0 && ctx->hp.H_P != P) || ctx->red_H_cap < H_bytes;
    plan.have_kept       = !plan.drop_all && ctx->hp.win.size() == (size_t) W;
    std::vector<int32_t> &r_off = plan.r_off, &c_off = plan.c_off, seen((size_t) P, -1);
    r_off.assign((size_t) nb + 1, 0), c_off.assign((size_t) nb + 1, 0);
    for (int w = 0; w < W; w++) {
        const std::vector<icg_hp_block> *kept = plan.have_kept ? &ctx->hp.win[(size_t) w] : nullptr;
        const int cnt = a.blk_off[w + 1] - a.blk_off[w], Pw = a.Pw[w];
        if (a.rebuild[w] && (Pw <= 0 || Pw > P)) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d: Pw = %d (1 .. %d)", me, w, Pw, P);
        bool any_keep = false;
        for (int b = a.blk_off[w]; b < a.blk_off[w + 1]; b++) {
            const int p = b - a.blk_off[w], nr = a.nr[b], nf = a.nf[b];
            if (nr <= 0 || nf <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d, block %d: %d x %d", me, w, p, nr, nf);
            if (nr > ICG_HOST_PART_MAX_NR)
                return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: window %d, block %d: %d residuals (at most %d)", me, w, p, nr, ICG_HOST_PART_MAX_NR);
            if ((int64_t) r_off[(size_t) b] + nr > INT32_MAX || (int64_t) c_off[(size_t) b] + nf > INT32_MAX)
                return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: window %d, block %d: more than 2^31 residuals or columns in one call", me, w, p);
            r_off[(size_t) b + 1] = r_off[(size_t) b] + nr, c_off[(size_t) b + 1] = c_off[(size_t) b] + nf;
            int idx[HP_FAMILIES]; // >= 0: the block is that member of the family's resident set
            size_t c0[HP_FAMILIES];
            for (int f = 0; f < HP_FAMILIES; f++) {
                idx[f] = F[f].of ? F[f].of[b] : -1, c0[f] = F[f].at;
                if (idx[f] >= 0) F[f].at += (size_t) nf; // (at most the columns of all blocks: below 2^31)
            }
            if (!a.rebuild[w]) continue;
            if (int rc = hp_validate_block(ctx, a, F, idx, c0, w, b, kept, seen, any_keep, plan)) return rc;
        }
        if (!a.rebuild[w]) continue;
        if (any_keep && (size_t) cnt != kept->size())
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %d: %d blocks, %zu kept, and a block keeps its Jacobian", me, w, cnt, kept->size());
        plan.n_rebuilt++, plan.out_cells += (size_t) Pw * (Pw + 1) / 2;
        plan.max_cells = std::max(plan.max_cells, Pw * (Pw + 1) / 2);
    }
    if (plan.res.size() > 65535) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: %zu prior blocks in one call (at most 65535)", me, plan.res.size());
    // the staged column list: one family's columns behind the other's, the blocks' offsets shifted to match
    size_t base[HP_FAMILIES];
    for (int f = 0; f < HP_FAMILIES; f++) {
        base[f] = plan.res_cols.size(), plan.n_res_cols += F[f].at;
        if (F[f].cols && !plan.res.empty()) plan.res_cols.insert(plan.res_cols.end(), F[f].cols, F[f].cols + F[f].at);
    }
    for (size_t k = 0; k < plan.res.size(); k++) plan.res[k].pc_off += (int32_t) base[plan.res_at[k][2]];
    return ICG_OK;
}

// Stage 2.  The kept Jacobians after this call (`next`: dense, window after window) and their buffer (*dst_out); what stays moves there, device to device.
static int hp_place_kept(icg_ctx *ctx, const hp_args &a, const hp_plan &plan, std::vector<std::vector<icg_hp_block>> &next, int *dst_out) {
    const int W     = a.W;
    icg_hp_kept &hp = ctx->hp;
    next.assign((size_t) W, {});
    int64_t total = 0;
    bool same     = plan.have_kept;
    for (int w = 0; w < W; w++) {
        std::vector<icg_hp_block> &nw = next[(size_t) w];
        if (a.rebuild[w])
            for (int b = a.blk_off[w]; b < a.blk_off[w + 1]; b++) nw.push_back({0, a.nr[b], a.nf[b]});
        else if (plan.have_kept)
            nw = hp.win[(size_t) w];
        same = same && nw.size() == hp.win[(size_t) w].size();
        for (size_t p = 0; p < nw.size(); p++) {
            if (same) same = hp.win[(size_t) w][p].off == total && hp.win[(size_t) w][p].nr == nw[p].nr && hp.win[(size_t) w][p].nf == nw[p].nf;
            nw[p].off = total;
            total += (int64_t) nw[p].nr * nw[p].nf;
        }
    }
    int rc;
    if (plan.drop_all) {
        icg_red_drop_host_parts(ctx, (size_t) W);
        if ((rc = icg_red_ensure_capacity(ctx, &ctx->d_red_H, &ctx->red_H_cap, sizeof(double) * (size_t) W * ((size_t) a.P * (a.P + 1) / 2)))) return rc;
    }
    const int dst = *dst_out = same ? hp.cur : 1 - hp.cur;
    if (same) return ICG_OK;
    // what stays moves into the other buffer, in runs that are contiguous on both sides
    const size_t bytes = sizeof(double) * (size_t) std::max<int64_t>(total, 1);
    if ((rc = icg_grow(ctx, (void **) &hp.d_J[dst], &hp.cap[dst], bytes, bytes + bytes / 4))) return rc;
    int64_t run_src = 0, run_dst = 0, run_n = 0;
    auto flush      = [&]() -> int {
        if (run_n) ICG_HIP(ctx, hipMemcpyAsync(hp.d_J[dst] + run_dst, hp.d_J[hp.cur] + run_src, sizeof(double) * (size_t) run_n, hipMemcpyDeviceToDevice, ctx->stream));
        run_n = 0;
        return 0;
    };
    for (int w = 0; w < W && plan.have_kept; w++)
        for (size_t p = 0; p < next[(size_t) w].size(); p++) {
            if (a.rebuild[w] && a.jac_off[(size_t) a.blk_off[w] + p] != -1) continue; // (shipped, or gathered from a resident block's source)
            const icg_hp_block &o = hp.win[(size_t) w][p], &n = next[(size_t) w][p];
            const int64_t len     = (int64_t) n.nr * n.nf;
            if (run_n && o.off == run_src + run_n && n.off == run_dst + run_n) {
                run_n += len;
                continue;
            }
            if ((rc = flush())) return rc;
            run_src = o.off, run_dst = n.off, run_n = len;
        }
    return flush();
}

struct hp_staged { // what hp_stage uploaded, as hp_launch passes it on
    std::vector<hp_win> wins;
    size_t n_copies;
    const hp_win *d_wins;
    const hp_blk *d_blks;
    const hp_copy *d_cp;
    const int32_t *d_cols, *d_pc;
    const hp_prior *d_pr;
    double *d_r;
    double *d_Jnew = nullptr;
};

// Stage 3.  The tables of the kernels, the columns, r and the shipped Jacobians into the arena, and up in one copy.
static int hp_stage(icg_ctx *ctx, const hp_args &a, const hp_family (&F)[HP_FAMILIES], hp_plan &plan, const std::vector<std::vector<icg_hp_block>> &next, icg_call &c, hp_staged &S) {
    const int W = a.W, nb = a.blk_off[W];
    const size_t slot = (size_t) a.P * (a.P + 1) / 2;
    std::vector<hp_blk> blks((size_t) nb);
    std::vector<hp_copy> copies;
    int64_t out_off = 0, src = 0;
    for (int w = 0; w < W; w++) {
        if (!a.rebuild[w]) continue;
        S.wins.push_back({w, a.Pw[w], a.blk_off[w], a.blk_off[w + 1], (int32_t) S.wins.size(), 0, (int64_t) ((size_t) w * slot), out_off});
        out_off += (int64_t) a.Pw[w] * (a.Pw[w] + 1) / 2;
        for (int b = a.blk_off[w]; b < a.blk_off[w + 1]; b++) {
            const icg_hp_block &n = next[(size_t) w][(size_t) (b - a.blk_off[w])];
            blks[(size_t) b]      = {n.off, plan.r_off[(size_t) b], plan.c_off[(size_t) b], a.nr[b], a.nf[b]};
            if (a.jac_off[b] >= 0) copies.push_back({src, n.off, (int64_t) a.nr[b] * a.nf[b]}), src += (int64_t) a.nr[b] * a.nf[b];
        }
    }
    for (size_t k = 0; k < plan.res.size(); k++) plan.res[k].Jd_off = next[(size_t) plan.res_at[k][0]][(size_t) plan.res_at[k][1]].off;
    const size_t n_r = (size_t) plan.r_off[(size_t) nb], n_c = (size_t) plan.c_off[(size_t) nb], ship_doubles = plan.ship_doubles;
    int rc;
    if ((rc = c.reserve(sizeof(hp_win) * S.wins.size() + sizeof(hp_blk) * blks.size() + sizeof(hp_copy) * copies.size() + sizeof(hp_prior) * plan.res.size() +
                        sizeof(int32_t) * (n_c + plan.n_res_cols) + sizeof(double) * (n_r + ship_doubles + 2 * (size_t) plan.n_rebuilt * a.P + plan.out_cells) + 20 * 256)))
        return rc;
    S.n_copies = copies.size();
    S.d_wins   = c.in(S.wins.data(), S.wins.size());
    S.d_blks   = c.in(blks.data(), blks.size());
    S.d_cp     = c.in(copies.data(), copies.size());
    S.d_cols   = c.in(a.cols, n_c);
    S.d_pr     = c.in(plan.res.data(), plan.res.size());
    S.d_pc     = plan.res.empty() ? nullptr : c.in(plan.res_cols.data(), plan.res_cols.size());
    if (std::none_of(F, F + HP_FAMILIES, [](const hp_family &G) { return G.of != nullptr; })) {
        S.d_r = c.in(a.r, n_r);
    } else {
        // The slots of the resident blocks (of every window, rebuilt or not) are placed but not read from the caller: staged block by block,
        // like the shipped Jacobians below.  Whatever bytes the arena holds there go up with the rest; for the rebuilt windows
        // k_host_part_prior overwrites them on the device, in stream order behind the upload and ahead of k_host_part, and the blocks of
        // the other windows are not consumed.
        double *h = c.stage<double>(n_r, &S.d_r);
        if (!h) return c.overflowed();
        for (int b = 0; b < nb; b++)
            if (std::none_of(F, F + HP_FAMILIES, [b](const hp_family &G) { return G.of && G.of[b] >= 0; })) memcpy(h + plan.r_off[(size_t) b], a.r + plan.r_off[(size_t) b], sizeof(double) * (size_t) a.nr[b]);
    }
    if (ship_doubles) { // the shipped Jacobians, block after block
        double *h = c.stage<double>(ship_doubles, &S.d_Jnew);
        if (!h) return c.overflowed();
        for (int w = 0; w < W; w++)
            for (int b = a.blk_off[w]; a.rebuild[w] && b < a.blk_off[w + 1]; b++)
                if (a.jac_off[b] >= 0) memcpy(h, a.J + a.jac_off[b], sizeof(double) * (size_t) a.nr[b] * a.nf[b]), h += (size_t) a.nr[b] * a.nf[b];
    }
    return c.seal();
}

// Stage 4.  The outputs, the three kernels, and once they are through the call's kept Jacobians and parts become the context's.
static int hp_launch(icg_ctx *ctx, const hp_args &a, const hp_plan &plan, std::vector<std::vector<icg_hp_block>> &next, int dst, icg_call &c, const hp_staged &S) {
    const int W = a.W, P = a.P;
    icg_hp_kept &hp = ctx->hp;
    // s and diag of the rebuilt windows only: the rows of the others are not the call's to write
    double *d_s = c.out((double *) nullptr, (size_t) plan.n_rebuilt * P), *d_dg = c.out((double *) nullptr, (size_t) plan.n_rebuilt * P);
    for (const hp_win &hw : S.wins) {
        c.outs.push_back({(void *) (a.host_s + (size_t) hw.w * P), (size_t) (reinterpret_cast<char *>(d_s + (size_t) hw.slot * P) - ctx->d_arena), sizeof(double) * (size_t) P, false});
        c.outs.push_back({(void *) (a.host_diag + (size_t) hw.w * P), (size_t) (reinterpret_cast<char *>(d_dg + (size_t) hw.slot * P) - ctx->d_arena), sizeof(double) * (size_t) P, false});
    }
    double *d_po = a.part_out ? c.out(a.part_out, plan.out_cells) : nullptr;
    ICG_LAUNCH_GUARD(c);
    // from here on the rebuilt windows' parts and the kept Jacobians are being replaced: a failure below leaves those windows without a part
    // and no window with a kept Jacobian
    for (int w = 0; w < W; w++)
        if (a.rebuild[w]) ctx->red_H_cols[(size_t) w] = 0;
    hp.win.clear();
    if (!plan.res.empty()) { // (its places among the kept Jacobians and in r are not the shipped blocks')
        icg_prof_scope ps(ctx, "host_part_prior");
        hipLaunchKernelGGL(k_host_part_prior, dim3((unsigned) ((plan.max_prior_nr + HP_PRIOR_ROWS - 1) / HP_PRIOR_ROWS), (unsigned) plan.res.size()), dim3(HP_THREADS), 0,
                           ctx->stream, S.d_pr, S.d_pc, hp.d_J[dst], S.d_r);
    }
    {
        icg_prof_scope ps(ctx, "host_part");
        if (S.n_copies) hipLaunchKernelGGL(k_host_part_keep, dim3((unsigned) S.n_copies), dim3(HP_THREADS), 0, ctx->stream, S.d_cp, S.d_Jnew, hp.d_J[dst]);
        hipLaunchKernelGGL(k_host_part, dim3((unsigned) ((plan.max_cells + HP_THREADS * HP_CPT - 1) / (HP_THREADS * HP_CPT)), (unsigned) plan.n_rebuilt), dim3(HP_THREADS), 0,
                           ctx->stream, S.d_wins, S.d_blks, S.d_cols, (const double *) hp.d_J[dst], S.d_r, P, ctx->d_red_H, d_s, d_dg, d_po);
    }
    ICG_HIP(ctx, hipGetLastError());
    if (int rc = c.finish()) return rc;
    hp.cur = dst, hp.H_P = P;
    hp.win.swap(next);
    for (int w = 0; w < W; w++)
        if (a.rebuild[w]) ctx->red_H_cols[(size_t) w] = a.Pw[w];
    return ICG_OK;
}

// ---- the exported entries (include/icgvins_hip.h): each hands hp_build what all of them take and an (of, cols) pair per family it has, in hp_families' order
#define HP_PARAMS                                                                                                                                                     \
    icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *rebuild, const int32_t *blk_off, const int32_t *nr, const int32_t *nf, const int32_t *cols,                 \
        const int64_t *jac_off, const double *J, const double *r, double *host_s, double *host_diag, double *part_out
#define HP_ARGS hp_args{nullptr, P, 0, Pw, blk_off, nr, nf, cols, rebuild, jac_off, J, r, host_s, host_diag, part_out}
typedef const int32_t *hp_table;

// The families beyond `tables` have none, as in a call of a wider entry with NULL for them: the messages name the entry of the widest family that has one.
static int hp_build(icg_ctx *ctx, hp_args a, std::initializer_list<std::array<hp_table, 2>> tables) {
    if (!ctx) return ICG_ERR_INVALID;
    hp_family F[HP_FAMILIES];
    std::copy(hp_families, hp_families + HP_FAMILIES, F);
    a.me = "icg_reproj_host_parts_build", a.W = ctx->part_w.W;
    hp_family *G = F;
    for (const std::array<hp_table, 2> &t : tables) G->of = t[0], G->cols = t[1], a.me = t[0] ? G->entry : a.me, G++;
    hp_plan plan;
    int rc, dst;
    if ((rc = hp_validate(ctx, a, F, plan))) return rc;
    if (plan.n_rebuilt == 0) return ICG_OK;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    std::vector<std::vector<icg_hp_block>> next;
    if ((rc = hp_place_kept(ctx, a, plan, next, &dst))) return rc;
    icg_call c(ctx);
    hp_staged S;
    if ((rc = hp_stage(ctx, a, F, plan, next, c, S))) return rc;
    return hp_launch(ctx, a, plan, next, dst, c, S);
}

extern "C" int icg_reproj_host_parts_build(HP_PARAMS) { return hp_build(ctx, HP_ARGS, {}); }

extern "C" int icg_reproj_host_parts_build_prior(HP_PARAMS, hp_table prior_of, hp_table prior_cols) { return hp_build(ctx, HP_ARGS, {{prior_of, prior_cols}}); }

extern "C" int icg_reproj_host_parts_build_preint(HP_PARAMS, hp_table prior_of, hp_table prior_cols, hp_table preint_of, hp_table preint_cols) {
    return hp_build(ctx, HP_ARGS, {{prior_of, prior_cols}, {preint_of, preint_cols}});
}

extern "C" int icg_reproj_host_parts_build_preint_odo(HP_PARAMS, hp_table prior_of, hp_table prior_cols, hp_table preint_of, hp_table preint_cols, hp_table preint_odo_of,
                                                      hp_table preint_odo_cols) {
    return hp_build(ctx, HP_ARGS, {{prior_of, prior_cols}, {preint_of, preint_cols}, {preint_odo_of, preint_odo_cols}});
}

extern "C" int icg_reproj_host_parts_build_nav(HP_PARAMS, hp_table prior_of, hp_table prior_cols, hp_table preint_of, hp_table preint_cols, hp_table preint_odo_of,
                                               hp_table preint_odo_cols, hp_table nav_of, hp_table nav_cols) {
    return hp_build(ctx, HP_ARGS, {{prior_of, prior_cols}, {preint_of, preint_cols}, {preint_odo_of, preint_odo_cols}, {nav_of, nav_cols}});
}
