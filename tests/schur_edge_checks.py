"""Reference and check bodies of the Schur-path edge suite: run through icgvins.Context on the oracle shim (test_schur_edges_cpu.py) and on the
HIP library (test_gpu_schur_edges.py).

The reference starts from the r and J that the library under test returned for the window, so it isolates what happens AFTER the factor
evaluation: from those exact doubles it forms H, b, inv, S, s, diag, delta_l, the landmark terms, h_ll, the cost and the chi-square mask in
np.longdouble, and next to every value the value's absolute-value sum A (the sum of |each product that enters the cell|) and a term count n_t.

Every output cell of the library is a fixed-order FP64 sum of products of entries of J and r (a cell of S: sums of such sums, multiplied by a
correctly rounded reciprocal, and one final subtraction).  Expanding a cell into its leaf products, every leaf picks up one factor (1 + d),
|d| <= 2^-53, per rounding on its way to the cell; n_t counts the roundings of the longest way, whatever order the additions are made in:
    H, b cells        two products per factor (one per residual row), at most one merge of partial sums per factor      n_t = 3 factors
    inv               h_ll (a sum of squares: A = h), the clamp product, the sum, the division                            n_h + 3
    S, s cells        the longest of: the camera cell itself | G_li * inv_l * G_lj (b_l) down the sum over the landmarks  + the subtraction
    delta_l, terms    the same rule along their formulas
so |got - exact| <= (n_t + 8) 2^-53 A, the textbook bound of a recursive sum; the eight spare roundings cover the second-order terms.  Derived,
not measured; where A is 0 (unowned columns, landmarks without an active factor, windows without factors) it asks for exactly 0.0."""
import numpy as np

import schur_edge_data as D

LD = np.longdouble
U = 2.0 ** -53
REF_SLACK = 1.0 if np.finfo(LD).nmant >= 63 else 2.0  # a reference without extended precision has a rounding of its own of the same size
_SLACK_NOTE = "" if REF_SLACK == 1.0 else " (bound doubled: np.longdouble has no extended mantissa here)"


def assert_cells(case, output, got, exp, A, nt):
    got = np.asarray(got, np.float64)
    exp, A = np.asarray(exp, LD), np.asarray(A, LD)
    assert got.shape == exp.shape == A.shape, (case, output, got.shape, exp.shape, A.shape)
    assert np.all(np.isfinite(got)), (case, output, "non-finite value")
    err = np.abs(got.astype(LD) - exp)
    bound = (np.asarray(nt, LD) + 8) * LD(U) * A * LD(REF_SLACK)
    bad = err > bound
    if bad.any():
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)).astype(np.float64)
        k = np.unravel_index(np.argmax(ratio), ratio.shape) if ratio.ndim else ()
        raise AssertionError(f"{case}: {output}{[int(i) for i in k]}: got {float(got[k])!r}, expected {float(exp[k])!r}, err / bound = {float(ratio[k]):.3g} "
                             f"(A = {float(A[k]):.6g}, {int(bad.sum())} of {bad.size} cells beyond the bound){_SLACK_NOTE}")


# ---- reference -----------------------------------------------------------------------------------------------------------------------------
def ref_normal(case, r, J, active):
    """H, b of the (P + L) system in long double from the library's own r and J, with A and n_t of every cell"""
    P, L = case["P"], case["L"]
    N = P + L
    H, AH, b, Ab = np.zeros((N, N), LD), np.zeros((N, N), LD), np.zeros(N, LD), np.zeros(N, LD)
    nH, nb = np.zeros((N, N), np.int64), np.zeros(N, np.int64)
    cp, ce, ct = case["col_pose"], int(case["col_ext"]), int(case["col_td"])
    for f in range(len(r)):
        if active is not None and not active[f]:
            continue
        cols, blocks = [], []
        for c0, blk in ((int(cp[case["idx_i"][f]]), J[f, 0:14].reshape(2, 7)[:, :6]), (int(cp[case["idx_j"][f]]), J[f, 14:28].reshape(2, 7)[:, :6]),
                        (ce, J[f, 28:42].reshape(2, 7)[:, :6]), (P + int(case["idx_lm"][f]), J[f, 42:44].reshape(2, 1)), (ct, J[f, 44:46].reshape(2, 1))):
            if c0 >= 0:
                cols.extend(range(c0, c0 + blk.shape[1]))
                blocks.append(blk)
        Jr = np.concatenate(blocks, axis=1).astype(LD)
        prod = Jr[:, :, None] * Jr[:, None, :]
        ix = np.ix_(cols, cols)
        H[ix] += prod[0] + prod[1]
        AH[ix] += np.abs(prod[0]) + np.abs(prod[1])
        nH[ix] += 3
        pr = Jr * r[f].astype(LD)[:, None]
        b[cols] -= pr[0] + pr[1]
        Ab[cols] += np.abs(pr[0]) + np.abs(pr[1])
        nb[cols] += 3
    return dict(H=H, AH=AH, nH=nH, b=b, Ab=Ab, nb=nb)


def ref_inv(case, nrm, damp, min_diag, max_diag):
    P = case["P"]
    h = np.diag(nrm["H"])[P:]
    clamped = np.minimum(np.maximum(h, LD(min_diag)), LD(max_diag))
    pos = h > 0
    inv = np.where(pos, 1 / np.where(pos, h + clamped * LD(damp), 1), 0).astype(LD)
    branch = np.where(~pos, -1, np.where(h < min_diag, 0, np.where(h > max_diag, 2, 1)))  # which clamp branch a landmark takes
    return dict(h=h, inv=inv, n_inv=np.diag(nrm["nH"])[P:] + 3, dl=np.where(pos, clamped * LD(damp), 0).astype(LD), branch=branch)


def ref_schur(case, nrm, iv):
    P, L = case["P"], case["L"]
    H, AH, nH, b, Ab, nb = (nrm[k] for k in ("H", "AH", "nH", "b", "Ab", "nb"))
    G, AG, nG = H[P:, :P], AH[P:, :P], nH[P:, :P]
    inv, n_inv = iv["inv"], iv["n_inv"]
    on = (inv > 0)[:, None] & (AG > 0)
    S = H[:P, :P] - G.T @ (inv[:, None] * G)
    AS = AH[:P, :P] + AG.T @ (inv[:, None] * AG)
    s = b[:P] - G.T @ (inv * b[P:])
    As = Ab[:P] + AG.T @ (inv * Ab[P:])
    nS_sum, ns_sum = np.zeros((P, P), np.int64), np.zeros(P, np.int64)
    for l in range(L):
        m = on[l]
        nS_sum = np.maximum(nS_sum, np.where(m[:, None] & m[None, :], nG[l][:, None] + nG[l][None, :] + n_inv[l], 0))
        ns_sum = np.maximum(ns_sum, np.where(m, nG[l] + n_inv[l] + nb[P + l], 0))
    cnt = on.astype(np.int64)
    nS = np.maximum(nH[:P, :P], nS_sum + cnt.T @ cnt + 3) + 1
    ns = np.maximum(nb[:P], ns_sum + cnt.sum(0) + 3) + 1
    return dict(S=S, AS=AS, nS=nS, s=s, As=As, ns=ns, diag=np.diag(H)[:P], Adiag=np.diag(AH)[:P], ndiag=np.diag(nH)[:P])


def ref_backsub(case, nrm, iv, dc):
    P, L = case["P"], case["L"]
    H, AH, nH, b, Ab, nb = (nrm[k] for k in ("H", "AH", "nH", "b", "Ab", "nb"))
    G, AG, nG = H[P:, :P], AH[P:, :P], nH[P:, :P]
    inv, n_inv = iv["inv"], iv["n_inv"]
    dcl = np.asarray(dc, np.float64).astype(LD)
    dl = (b[P:] - G @ dcl) * inv
    Adl = (Ab[P:] + AG @ np.abs(dcl)) * inv
    ndl = np.maximum(nb[P:], (nG.max(axis=1) if P else 0) + 1 + (AG > 0).sum(axis=1)) + 1 + n_inv + 1
    pos = inv > 0
    t0, At0 = (b[P:] ** 2 * inv)[pos].sum(), (Ab[P:] ** 2 * inv)[pos].sum()
    t1, At1 = (iv["dl"] * dl * dl)[pos].sum(), (iv["dl"] * Adl * Adl)[pos].sum()
    npos = int(pos.sum())
    nt0 = (2 * nb[P:][pos].max() + n_inv[pos].max() + 2 + npos) if npos else 0
    nt1 = (2 * ndl[pos].max() + n_inv[pos].max() + 4 + npos) if npos else 0
    return dict(dl=dl, Adl=Adl, ndl=ndl, terms=np.array([t0, t1], LD), Aterms=np.array([At0, At1], LD), nterms=np.array([nt0, nt1]), zero=~pos)


def ref_cost(r, active, huber):
    """0.5 sum rho with the Huber rule of k_reproj_cost_w on (possibly corrected) residuals; also how many factors took each branch"""
    rl = np.asarray(r, np.float64).astype(LD)
    q = rl[:, 0] ** 2 + rl[:, 1] ** 2
    act = np.ones(len(q), bool) if active is None else np.asarray(active, bool)
    out = (q > LD(huber) ** 2) & (huber > 0)
    val = np.where(out, 2 * q - LD(huber) ** 2, q)
    A = np.where(out, 2 * q + LD(huber) ** 2, q)
    return (0.5 * val[act]).sum(), (0.5 * A[act]).sum(), int(act.sum()) + 6, int((out & act).sum()), int((~out & act).sum())


def chi2_thresholds(r):
    """thresholds midway between neighbouring values of the sorted r0^2 + r1^2 (below the minimum, in the middle, above the maximum): no
    factor sits within 1e-12 relative of one, so the contraction of r0 * r0 + r1 * r1 on the device cannot decide a case"""
    rl = np.asarray(r, np.float64).astype(LD)
    q = rl[:, 0] ** 2 + rl[:, 1] ** 2
    qs = np.sort(q)
    th = [float(qs[0] / 2), float(qs[-1] * 2)]
    for k in sorted({len(qs) // 4, len(qs) // 2, (3 * len(qs)) // 4}):
        if 0 < k < len(qs):
            th.append(float((qs[k - 1] + qs[k]) / 2))
    good = [t for t in th if np.all(np.abs(q - LD(t)) > LD(1e-12) * LD(t))]
    assert len(good) >= 2, "no usable chi-square threshold"
    return q, good


# ---- check bodies --------------------------------------------------------------------------------------------------------------------------
def _eval(ctx, case):
    ctx.reproj_set_factors(case["obs_soa"], case["idx_i"], case["idx_j"], case["idx_lm"])
    r, J = ctx.reproj_eval_resident(case["poses"], case["ext"], case["invdepth"], case["td"], huber=case["huber"], fetch=True)
    assert np.array_equal(ctx.reproj_fetch_residuals(), r), (case["name"], "icg_reproj_fetch_residuals differs from the fetched residuals")
    return r, J


def _clamps(case, nrm):
    if not case["clamp_percentiles"]:
        return case["min_diag"], case["max_diag"]
    h = np.diag(nrm["H"])[case["P"]:].astype(np.float64)
    lo, hi = np.percentile(h[h > 0], case["clamp_percentiles"])
    return float(lo), float(hi)


def _compare_system(name, tag, S, s, dg, rs, symmetric, lower_only=False):
    P = len(s)
    if lower_only:
        low = np.arange(P)[:, None] >= np.arange(P)[None, :]
        assert_cells(name, tag + "S_view(lower)", np.where(low, S, 0.0), np.where(low, rs["S"], 0), np.where(low, rs["AS"], 0), rs["nS"])
    else:
        assert_cells(name, tag + "S", S, rs["S"], rs["AS"], rs["nS"])
        if symmetric:
            assert np.array_equal(S, S.T), (name, tag + "S is not exactly symmetric")
    assert_cells(name, tag + "s", s, rs["s"], rs["As"], rs["ns"])
    assert_cells(name, tag + "diag", dg, rs["diag"], rs["Adiag"], rs["ndiag"])


def _compare_backsub(name, tag, dl, terms, rb):
    assert_cells(name, tag + "delta_l", dl, rb["dl"], rb["Adl"], rb["ndl"])
    assert np.all(np.asarray(dl)[rb["zero"]] == 0.0), (name, tag + "delta_l of a landmark with inv == 0 is not exactly 0")
    assert_cells(name, tag + "terms", terms, rb["terms"], rb["Aterms"], rb["nterms"])
    if rb["zero"].all():
        assert terms[0] == 0.0 and terms[1] == 0.0, (name, tag + "terms of a window without a live landmark")


def check_case(ctx, case, device, stats=None):
    """one window through the single-window entry points: icg_reproj_accumulate_normal, icg_reproj_schur at every damping of the case (and
    reassemble = 0 at the later ones), icg_reproj_landmark_diag, icg_reproj_backsub, icg_reproj_cost.  device: the library is the HIP one
    (exact symmetry and bit-for-bit repeatability are asserted there)."""
    name, P, L = case["name"], case["P"], case["L"]
    r, J = _eval(ctx, case)
    # H and b of the whole system, every factor (the entry point takes no mask)
    full = ref_normal(case, r, J, None)
    Hgot, bgot = ctx.reproj_accumulate_normal(P + L, case["col_pose"], case["col_ext"], P + np.arange(L, dtype=np.int32), case["col_td"])
    assert_cells(name, "H", Hgot, full["H"], full["AH"], full["nH"])
    assert_cells(name, "b", bgot, full["b"], full["Ab"], full["nb"])
    act = case["active"]
    nrm = full if act is None else ref_normal(case, r, J, act)
    min_diag, max_diag = _clamps(case, nrm)
    cost_exp, cost_A, cost_n, n_out, n_in = ref_cost(r, act, case["huber"])
    rng = np.random.RandomState(17)
    dc = rng.normal(0, 1e-3, P)
    first = None
    for damp in case["damps"]:
        iv = ref_inv(case, nrm, damp, min_diag, max_diag)
        rs, rb = ref_schur(case, nrm, iv), ref_backsub(case, nrm, iv, dc)
        tag = f"damp={damp:g}: "
        fresh = ctx.reproj_schur(P, case["col_pose"], case["col_ext"], case["col_td"], active=act, damp=damp, min_diag=min_diag, max_diag=max_diag)
        S, s, dg, cost = fresh
        _compare_system(name, tag, S, s, dg, rs, symmetric=device)
        assert_cells(name, tag + "cost", np.float64(cost), cost_exp, cost_A, cost_n)
        assert_cells(name, tag + "h_ll", ctx.reproj_landmark_diag(L), iv["h"], np.diag(nrm["AH"])[P:], np.diag(nrm["nH"])[P:])
        dl, terms = ctx.reproj_backsub(P, dc, L)
        _compare_backsub(name, tag, dl, terms, rb)
        if device:
            again = ctx.reproj_schur(P, case["col_pose"], case["col_ext"], case["col_td"], active=act, damp=damp, min_diag=min_diag, max_diag=max_diag)
            for a, b_, what in zip(fresh, again, ("S", "s", "diag", "cost")):
                assert np.array_equal(np.asarray(a), np.asarray(b_)), (name, tag + what + ": the same call repeated gives other bits")
            dl2, terms2 = ctx.reproj_backsub(P, dc, L)
            assert np.array_equal(dl, dl2) and np.array_equal(terms, terms2), (name, tag + "back-substitution repeated gives other bits")
        if first is not None:
            # the systems left by the first assembly, damped anew, against the fresh assembly above (bit for bit on the device)
            ctx.reproj_schur(P, case["col_pose"], case["col_ext"], case["col_td"], active=act, damp=first, min_diag=min_diag, max_diag=max_diag)
            S0, s0, dg0, _ = ctx.reproj_schur(P, case["col_pose"], case["col_ext"], case["col_td"], active=act, reassemble=False, damp=damp,
                                              min_diag=min_diag, max_diag=max_diag)
            _compare_system(name, tag + "reassemble=0: ", S0, s0, dg0, rs, symmetric=device)
            dl0, terms0 = ctx.reproj_backsub(P, dc, L)
            _compare_backsub(name, tag + "reassemble=0: ", dl0, terms0, rb)
            if device:
                for a, b_, what in ((S0, S, "S"), (s0, s, "s"), (dg0, dg, "diag"), (dl0, dl, "delta_l"), (terms0, terms, "terms")):
                    assert np.array_equal(a, b_), (name, tag + what + ": reassemble = 0 at a new damping differs from a fresh assembly")
        else:
            first = damp
        if stats is not None:
            stats.setdefault("branches", set()).update(int(v) for v in iv["branch"])
    ctx.reproj_eval_resident(case["poses"], case["ext"], case["invdepth"], case["td"], want_jac=False, huber=case["huber"], fetch=False)
    assert_cells(name, "icg_reproj_cost", np.float64(ctx.reproj_cost(act)), cost_exp, cost_A, cost_n)
    if stats is not None:
        stats["huber_outliers"], stats["huber_inliers"] = n_out, n_in
        stats["inv_zero"] = int((ref_inv(case, nrm, 0.0, min_diag, max_diag)["inv"] == 0).sum())
    return r


def check_chi2(ctx, case):
    """icg_reproj_chi2_cull against the mask formed from the library's own residuals, exactly: thresholds below the minimum, in the middle and
    above the maximum of r0^2 + r1^2, with a mask of ones and with a mask that already holds zeros"""
    r, _ = _eval(ctx, case)
    q, ths = chi2_thresholds(r)
    n = len(q)
    rng = np.random.RandomState(5)
    holes = (rng.uniform(0, 1, n) > 0.3).astype(np.uint8)
    seen = set()
    for th in ths:
        for mask_in in (np.ones(n, np.uint8), holes):
            exp = (mask_in.astype(bool) & ~(q > LD(th))).astype(np.uint8)
            got = ctx.reproj_chi2_cull(th, mask_in)
            assert got.dtype == np.uint8 and np.array_equal(got, exp), (case["name"], "chi2", th, np.nonzero(got != exp)[0][:8])
            seen.add((bool(exp.all()), bool(exp.any())))
    return seen


def check_refusal(ctx, case, capacity_code=-5):
    """a reduced system wider than the limit is refused with the capacity code and leaves the context usable (the caller runs a case next)"""
    import icgvins
    assert case["P"] > D.P_LIMIT
    _eval(ctx, case)
    try:
        ctx.reproj_schur(case["P"], case["col_pose"], case["col_ext"], case["col_td"], damp=1e-4)
    except icgvins.IcgError as e:
        assert f"rc={capacity_code}:" in str(e), e
    else:
        raise AssertionError(f"{case['name']}: P = {case['P']} was not refused")


def concat(cases):
    """the windows of `cases` as one resident set: poses indexed globally, landmarks and factors contiguous per window"""
    pose_off = np.concatenate([[0], np.cumsum([c["n_poses"] for c in cases])]).astype(np.int64)
    lm_off = np.concatenate([[0], np.cumsum([c["L"] for c in cases])]).astype(np.int32)
    fac_off = np.concatenate([[0], np.cumsum([len(c["idx_i"]) for c in cases])]).astype(np.int32)
    P = cases[0]["P"]
    assert all(c["P"] == P for c in cases)
    act = np.concatenate([np.ones(len(c["idx_i"]), np.uint8) if c["active"] is None else c["active"] for c in cases])
    return dict(pose_off=pose_off, lm_off=lm_off, fac_off=fac_off, P=P, obs=np.concatenate([c["obs_soa"] for c in cases], axis=1),
                ii=np.concatenate([c["idx_i"] + pose_off[k] for k, c in enumerate(cases)]).astype(np.int32),
                jj=np.concatenate([c["idx_j"] + pose_off[k] for k, c in enumerate(cases)]).astype(np.int32),
                ll=np.concatenate([c["idx_lm"] + lm_off[k] for k, c in enumerate(cases)]).astype(np.int32),
                poses=np.concatenate([c["poses"] for c in cases]), ext=np.stack([c["ext"] for c in cases]),
                inv=np.concatenate([c["invdepth"] for c in cases]), td=np.array([c["td"] for c in cases]),
                col_pose=np.concatenate([c["col_pose"] for c in cases]).astype(np.int32), col_ext=np.array([c["col_ext"] for c in cases], np.int32),
                col_td=np.array([c["col_td"] for c in cases], np.int32), active=act)


def check_batch(make_ctx, cases, device, damp1=None, damp2=None, stats=None):
    """the windows of `cases` in one launch of the many-window entry points (icg_reproj_schur_windows, _view, _backsub_windows,
    _landmark_diag_windows, _cost_windows) against the long-double reference of each window; on the device also bit for bit against the same
    window alone in a context of its own, against the same call repeated, and reassemble = 0 at a new damping against a fresh assembly"""
    W = len(cases)
    B = concat(cases)
    P = B["P"]
    huber = cases[0]["huber"]
    damp1 = np.full(W, 1e-4) if damp1 is None else np.asarray(damp1, np.float64)
    damp2 = damp1 * 7.0 + 1e-5 if damp2 is None else np.asarray(damp2, np.float64)
    singles, rJ = [], []
    for c in cases:
        if len(c["idx_i"]) == 0:
            singles.append(None), rJ.append((np.zeros((0, 2)), np.zeros((0, 46))))
            continue
        ctx = make_ctx()
        singles.append(ctx)
        rJ.append(_eval(ctx, c))
    ctxb = make_ctx()
    try:
        ctxb.reproj_set_factors(B["obs"], B["ii"], B["jj"], B["ll"])
        ctxb.reproj_set_windows(B["fac_off"], B["lm_off"])
        ctxb.reproj_eval_windows(B["poses"], B["ext"], B["inv"], B["td"], huber=huber)
        r_all = np.concatenate([r for r, _ in rJ])
        # the per-factor evaluation does not depend on the call it is made through: the reference may use each window's own fetch
        assert np.array_equal(ctxb.reproj_fetch_residuals(), r_all), "residuals of the batched evaluation differ from the single-window ones"
        nrms = [ref_normal(c, rJ[k][0], rJ[k][1], c["active"]) for k, c in enumerate(cases)]
        clamp_src = next((k for k, c in enumerate(cases) if c["clamp_percentiles"]), None)
        min_diag, max_diag = _clamps(cases[clamp_src], nrms[clamp_src]) if clamp_src is not None else (1e-6, 1e32)
        rng = np.random.RandomState(23)
        dc = rng.normal(0, 1e-3, (W, P))
        args = (P, B["col_pose"], B["col_ext"], B["col_td"])

        def compare(tag, damp, out, dl, terms, hll, lower_only=False):
            S, s, dg, cost = out
            for k, c in enumerate(cases):
                iv = ref_inv(c, nrms[k], damp[k], min_diag, max_diag)
                rs, rb = ref_schur(c, nrms[k], iv), ref_backsub(c, nrms[k], iv, dc[k])
                nm = f"{c['name']} (window {k} of {W})"
                _compare_system(nm, tag, S[k], s[k], dg[k], rs, symmetric=device, lower_only=lower_only)
                l0, l1 = B["lm_off"][k], B["lm_off"][k + 1]
                if dl is not None:
                    _compare_backsub(nm, tag, dl[l0:l1], terms[k], rb)
                if hll is not None:
                    assert_cells(nm, tag + "h_ll", hll[l0:l1], iv["h"], np.diag(nrms[k]["AH"])[P:], np.diag(nrms[k]["nH"])[P:])
                if cost is not None:
                    ce, cA, cn, _, _ = ref_cost(rJ[k][0], c["active"], huber)
                    assert_cells(nm, tag + "cost", np.float64(cost[k]), ce, cA, cn)
                if stats is not None:
                    stats.setdefault("branches", set()).update(int(v) for v in iv["branch"])

        out1 = ctxb.reproj_schur_windows(*args, active=B["active"], damp=damp1, min_diag=min_diag, max_diag=max_diag)
        hll = ctxb.reproj_landmark_diag_windows(len(B["inv"]))
        dl1, terms1 = ctxb.reproj_backsub_windows(P, dc, len(B["inv"]))
        compare("batch: ", damp1, out1, dl1, terms1, hll)
        costs = ctxb.reproj_cost_windows(B["active"])
        for k, c in enumerate(cases):
            ce, cA, cn, _, _ = ref_cost(rJ[k][0], c["active"], huber)
            assert_cells(c["name"], "icg_reproj_cost_windows", np.float64(costs[k]), ce, cA, cn)
        ctxb.reproj_reserve_windows(P)
        outv = ctxb.reproj_schur_windows_view(*args, active=B["active"], damp=damp1, min_diag=min_diag, max_diag=max_diag)
        compare("view: ", damp1, outv, None, None, None, lower_only=True)
        if device:
            low = np.arange(P)[:, None] >= np.arange(P)[None, :]
            assert np.array_equal(np.where(low, outv[0], 0.0), np.where(low, out1[0], 0.0)), "view and copying call differ in the lower triangle"
            for a, b_, what in zip(outv[1:], out1[1:], ("s", "diag", "cost")):
                assert np.array_equal(a, b_), ("view and copying call differ", what)
            # a window alone == the same window in the batch
            for k, c in enumerate(cases):
                if singles[k] is None:
                    continue
                S1, s1, dg1, cost1 = singles[k].reproj_schur(P, c["col_pose"], c["col_ext"], c["col_td"], active=c["active"], damp=damp1[k],
                                                              min_diag=min_diag, max_diag=max_diag)
                d1, t1 = singles[k].reproj_backsub(P, dc[k], c["L"])
                l0, l1 = B["lm_off"][k], B["lm_off"][k + 1]
                for a, b_, what in ((S1, out1[0][k], "S"), (s1, out1[1][k], "s"), (dg1, out1[2][k], "diag"), (np.float64(cost1), out1[3][k], "cost"),
                                    (d1, dl1[l0:l1], "delta_l"), (t1, terms1[k], "terms")):
                    assert np.array_equal(a, b_), (c["name"], what, "alone and in a batch differ in bits")
            out1b = ctxb.reproj_schur_windows(*args, active=B["active"], damp=damp1, min_diag=min_diag, max_diag=max_diag)
            for a, b_, what in zip(out1, out1b, ("S", "s", "diag", "cost")):
                assert np.array_equal(a, b_), ("the same batched call repeated gives other bits", what)
        # re-damping without re-assembly (every window), against the reference and against a fresh assembly at that damping
        out2 = ctxb.reproj_schur_windows(*args, active=B["active"], reassemble=np.zeros(W, np.uint8), damp=damp2, min_diag=min_diag, max_diag=max_diag)
        dl2, terms2 = ctxb.reproj_backsub_windows(P, dc, len(B["inv"]))
        compare("batch, reassemble=0: ", damp2, (out2[0], out2[1], out2[2], None), dl2, terms2, None)
        if device:
            out3 = ctxb.reproj_schur_windows(*args, active=B["active"], damp=damp2, min_diag=min_diag, max_diag=max_diag)
            dl3, terms3 = ctxb.reproj_backsub_windows(P, dc, len(B["inv"]))
            for a, b_, what in ((out2[0], out3[0], "S"), (out2[1], out3[1], "s"), (out2[2], out3[2], "diag"), (dl2, dl3, "delta_l"), (terms2, terms3, "terms")):
                assert np.array_equal(a, b_), ("reassemble = 0 at a new damping differs from a fresh assembly", what)
    finally:
        for c in singles + [ctxb]:
            if c is not None:
                c.close()
