"""Inputs for the Schur-path edge suite (tests/schur_edge_checks.py, test_schur_edges_cpu.py, test_gpu_schur_edges.py): windows that sit on the
structural edges of csrc/reproj_asm.hip and csrc/reproj_schur.hip — the fixed-order assembly (k_asm_runs, k_asm_camera, k_asm_landmarks), the landmark
elimination (k_schur_inv_w, k_schur_reduce_w, k_schur_backsub_w, k_terms_reduce_w), k_reproj_cost_w, k_lm_diag_w and k_reproj_chi2.

A case is one window: a factor list (ordered pose pairs, duplicates and run lengths are explicit), a column layout (col_pose, col_ext, col_td, P)
and an optional active mask.  The poses stand on an arc and look at one landmark cloud, so every (pose, landmark) pair has positive depth whatever
the pose count.  expected_plan() restates in plain Python what the host derives from a case (asm_plan_build / schur_impl): the tests assert with it
that a case is where it claims to be."""
import numpy as np

import reproj_data as rd

ASML_FB = 64   # factors per staging pass of k_asm_landmarks
ASM_SUB = 16   # factors per staging pass of k_asm_runs
SCH_LT = 32    # landmark rows per pass of k_schur_reduce_w ...
SCH_ELEMS = 3072  # ... as long as LT * 4 TQ stays within this many staged elements
P_LIMIT = 512

_QIC = np.array([0.497766, 0.502679, 0.501396, 0.498141])
_QIC = _QIC / np.linalg.norm(_QIC)
_TIC = np.array([0.074, -0.030, 0.128])
_F = 787.0


# ---- column layouts ------------------------------------------------------------------------------------------------------------------------
def layout(n_poses, tokens):
    """tokens in column order: ("pose", k) six columns, ("ext",) six, ("td",) one, ("gap", n) n columns nobody owns.  A pose that is not named
    is constant (col_pose = -1)."""
    col_pose, col_ext, col_td, c = np.full(n_poses, -1, np.int32), -1, -1, 0
    for tok in tokens:
        if tok[0] == "pose":
            assert col_pose[tok[1]] < 0
            col_pose[tok[1]] = c
            c += 6
        elif tok[0] == "ext":
            assert col_ext < 0
            col_ext = c
            c += 6
        elif tok[0] == "td":
            assert col_td < 0
            col_td = c
            c += 1
        else:
            c += tok[1]
    return dict(col_pose=col_pose, col_ext=col_ext, col_td=col_td, P=c)


def plain_layout(n_poses, spare=0, ext=True, td=True, const=(), spare_first=False):
    """poses in order, then ext, then td; `spare` unowned columns at the end (or in front of everything)"""
    tok = [("pose", k) for k in range(n_poses) if k not in const] + ([("ext",)] if ext else []) + ([("td",)] if td else [])
    gap = [("gap", spare)] if spare else []
    return layout(n_poses, gap + tok if spare_first else tok + gap)


# ---- factor lists --------------------------------------------------------------------------------------------------------------------------
def spread_factors(n_poses, L, per_pose, rng):
    """every pose observes `per_pose` landmarks; a landmark's reference is its home pose (l mod n_poses) unless that is the observer: few
    landmarks, every pose used, a few hundred factors at 84 poses"""
    fac = []
    for j in range(n_poses):
        for l in rng.choice(L, min(per_pose, L), replace=False):
            i = int(l) % n_poses
            if i == j:
                i = (j + 1 + rng.randint(0, n_poses - 1)) % n_poses
            fac.append((i, j, int(l)))
    order = rng.permutation(len(fac))
    return [fac[k] for k in order]


def run_factors(runs, L, rng):
    """runs: [((i, j), length)]: `length` factors of the ordered pair (i, j), landmarks drawn at random; the list is shuffled afterwards (the
    plan sorts it back into runs, keeping the list order inside a run)"""
    fac = []
    for (i, j), n in runs:
        fac += [(i, j, int(rng.randint(0, L))) for _ in range(n)]
    order = rng.permutation(len(fac))
    return [fac[k] for k in order]


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------
def make_case(name, n_poses, L, factors, lay, seed, active=None, huber=1.5, damps=(1e-4,), min_diag=1e-6, max_diag=1e32, pixel_noise=1.0,
              clamp_percentiles=None):
    """factors: list of (reference pose, observer pose, landmark).  Returns the dict every check body takes."""
    rng = np.random.RandomState(seed)
    center, radius = np.array([25.0, 0.0, 0.0]), 20.0
    th = np.linspace(-0.35, 0.35, n_poses) if n_poses > 1 else np.zeros(1)
    poses = np.zeros((n_poses, 7))
    for k in range(n_poses):
        poses[k, :3] = center - radius * np.array([np.cos(th[k]), np.sin(th[k]), 0.0]) + rng.normal(0, 0.05, 3)
        poses[k, 3:] = rd.quat_from_rotvec(np.array([rng.normal(0, 0.01), rng.normal(0, 0.01), th[k]]))
    Ric = rd.quat_to_R(_QIC)
    pw = center + rng.uniform(-4.0, 4.0, (max(L, 1), 3))
    pc = np.zeros((n_poses, max(L, 1), 3))  # landmark l in camera k
    for k in range(n_poses):
        Rk = rd.quat_to_R(poses[k, 3:])
        pc[k] = ((pw - poses[k, :3]) @ Rk - _TIC) @ Ric
    assert pc[:, :, 2].min() > 5.0  # every (pose, landmark) pair has positive depth
    invdepth = 1.0 / pc[np.arange(L) % n_poses, np.arange(L), 2] * (1 + rng.normal(0, 0.01, L)) if L else np.zeros(0)
    n = len(factors)
    obs = np.zeros((n, 15))
    for f, (i, j, l) in enumerate(factors):
        assert i != j and 0 <= l < L
        obs[f, 0:3] = [pc[i, l, 0] / pc[i, l, 2], pc[i, l, 1] / pc[i, l, 2], 1.0]
        obs[f, 3:6] = [pc[j, l, 0] / pc[j, l, 2] + rng.normal(0, pixel_noise / _F), pc[j, l, 1] / pc[j, l, 2] + rng.normal(0, pixel_noise / _F), 1.0]
        obs[f, 6:8], obs[f, 9:11] = rng.normal(0, 0.05, 2), rng.normal(0, 0.05, 2)
        obs[f, 12:15] = [0.001, 0.002, 1.5 / _F]
    fa = np.array(factors, np.int32).reshape(-1, 3)
    return dict(name=name, n_poses=n_poses, L=L, poses=poses, ext=np.concatenate([_TIC, _QIC]), td=0.003, invdepth=invdepth,
                obs_soa=np.ascontiguousarray(obs.T), idx_i=fa[:, 0].copy(), idx_j=fa[:, 1].copy(), idx_lm=fa[:, 2].copy(),
                active=None if active is None else np.asarray(active, np.uint8), huber=huber, damps=tuple(damps), min_diag=min_diag,
                max_diag=max_diag, clamp_percentiles=clamp_percentiles, **lay)


# ---- what the host derives -----------------------------------------------------------------------------------------------------------------
def red_lt(P):
    TQ = (P + 3) // 4
    return max(1, min(SCH_LT, SCH_ELEMS // (4 * TQ)))


def expected_plan(case):
    """K, run lengths, n_runs, TQ, NT, red_LT, the block list of the landmark rows and NB of one window (asm_plan_build, schur_impl).  NBmax and LB
    belong to the launch: expected_launch()."""
    ii, jj, ll = case["idx_i"], case["idx_j"], case["idx_lm"]
    used = sorted(set(ii.tolist()) | set(jj.tolist()))
    runs = {}
    for i, j in zip(ii.tolist(), jj.tolist()):
        runs[(i, j)] = runs.get((i, j), 0) + 1
    P = case["P"]
    owner = [None] * P

    def claim(col, width, code):
        if col < 0:
            return
        assert col + width <= P
        for x in range(width):
            assert owner[col + x] is None
            owner[col + x] = (code, x)

    for g in used:
        claim(int(case["col_pose"][g]), 6, ("pose", g))
    claim(int(case["col_ext"]), 6, ("ext",))
    claim(int(case["col_td"]), 1, ("td",))
    blocks, a = [], 0
    while a < P:
        o = owner[a]
        if o is None:
            w = 1
            while a + w < P and w < 6 and owner[a + w] is None:
                w += 1
            blocks.append(("gap", a, w))
            a += w
        elif o[0] == ("td",):
            a += 1
        else:
            blocks.append((o[0][0], a, 6))
            a += 6
    blocks.append(("td", int(case["col_td"]), 1))
    gaps, a = [], 0  # maximal runs of unowned columns
    while a < P:
        if owner[a] is None:
            b = a
            while b < P and owner[b] is None:
                b += 1
            gaps.append((a, b - a))
            a = b
        else:
            a += 1
    per_lm = np.bincount(ll, minlength=max(case["L"], 1)) if len(ll) else np.zeros(max(case["L"], 1), int)
    TQ = (P + 3) // 4
    return dict(K=len(used), runs=runs, run_lengths=sorted(runs.values()), n_runs=len(runs), TQ=TQ, NT=TQ * (TQ + 1) // 2, red_LT=red_lt(P),
                reduce_workgroups=(TQ * (TQ + 1) // 2 + 255) // 256, blocks=blocks, NB=len(blocks), gap_runs=gaps, owner=owner,
                factors_per_landmark=per_lm, n_factors=len(ii))


def expected_launch(cases):
    """the quantities that belong to one launch over `cases` (one window each): Kmax, NBmax and LB = 256 / NBmax of k_asm_landmarks"""
    plans = [expected_plan(c) for c in cases]
    NBmax = max(1, max(p["NB"] for p in plans))
    return dict(plans=plans, Kmax=max(1, max(p["K"] for p in plans)), NBmax=NBmax, LB=max(1, 256 // NBmax))


# ---- the named cases -----------------------------------------------------------------------------------------------------------------------
def _width_case(P, L, seed):
    """full pose blocks + ext + td and at most five spare columns (at the end; in front at P = 257, so that column 256 holds data)"""
    n_poses = (P - 7) // 6
    spare = P - 7 - 6 * n_poses
    assert 0 <= spare <= 5 and n_poses >= 2
    rng = np.random.RandomState(seed)
    return make_case(f"width_P{P}_L{L}", n_poses, L, spread_factors(n_poses, L, 3, rng), plain_layout(n_poses, spare, spare_first=P == 257), seed)


def width_cases():
    """(case, expected NT, expected reduce workgroups, expected LT)"""
    out = [(_width_case(88, 20, 100), 253, 1, 32), (_width_case(92, 20, 101), 276, 2, 32)]
    for P, LT, seed in ((96, 32, 110), (97, 30, 120)):
        out += [(_width_case(P, L, seed + k), None, 2, LT) for k, L in enumerate((LT - 1, LT, LT + 1, 2 * LT + 1))]
    out += [(_width_case(P, 20, 130 + P), None, None, SCH_ELEMS // (4 * ((P + 3) // 4))) for P in (255, 256, 257)]
    for P in (509, 510, 511, 512):
        out += [(_width_case(P, L, 140 + 4 * P + k), None, 33, 6) for k, L in enumerate((5, 6, 7, 13))]
    return out


def over_limit_case():
    return _width_case(513, 7, 150)


MID_POSES = 9  # P = 9 * 6 + 7 + 2 = 63 for the landmark-count and run cases


def landmark_count_cases():
    rng = np.random.RandomState(200)
    lay = plain_layout(MID_POSES, 2)
    one = make_case("L1", MID_POSES, 1, spread_factors(MID_POSES, 1, 1, rng), lay, 201)
    # landmark 2 has no factor at all; every factor of landmark 5 is inactive
    fac = [f for f in spread_factors(MID_POSES, 12, 4, rng) if f[2] != 2]
    act = np.array([0 if f[2] == 5 else 1 for f in fac], np.uint8)
    assert any(f[2] == 5 for f in fac)
    holes = make_case("empty_landmarks", MID_POSES, 12, fac, lay, 202, active=act)
    return [one, holes]


def empty_window_batch():
    """a window with L = 0 and no factors between two ordinary windows (same P)"""
    rng = np.random.RandomState(210)
    lay = plain_layout(MID_POSES, 2)
    a = make_case("batch_a", MID_POSES, 10, spread_factors(MID_POSES, 10, 3, rng), lay, 211)
    e = make_case("batch_empty", MID_POSES, 0, [], lay, 212)
    b = make_case("batch_b", MID_POSES, 14, spread_factors(MID_POSES, 14, 4, rng), lay, 213)
    return [a, e, b]


def run_cases():
    rng = np.random.RandomState(300)
    out = []
    # run lengths 1, 15, 16, 17, 32, 33 in one window; (0, 1) and (1, 0) both present; n_runs = 6 + 1 = 7 (mod 4 = 3)
    runs = [((0, 1), 1), ((1, 0), 15), ((1, 2), 16), ((2, 1), 17), ((0, 3), 32), ((3, 2), 33), ((4, 0), 20)]
    fac = run_factors(runs, 15, rng)
    act = np.ones(len(fac), np.uint8)
    for f, (i, j, l) in enumerate(fac):
        if (i, j) == (4, 0):
            act[f] = 0  # a run with every factor inactive
    mid = [f for f, (i, j, l) in enumerate(fac) if (i, j) == (3, 2)]
    act[mid[5:9]] = 0  # inactive factors in the middle of the first pass of a 33-factor run
    act[mid[20]] = 0   # and one inside the second pass
    out.append(make_case("run_lengths", 5, 15, fac, plain_layout(5, 1), 301, active=act))
    for K in (2, 3, 4, 5, 8, 9):
        pairs = [(i, j) for i in range(K) for j in range(K) if i != j]
        sel = [pairs[k] for k in rng.permutation(len(pairs))[:max(1, min(len(pairs), K + 1))]]
        # every pose appears in some run
        for p in range(K):
            if not any(p in s for s in sel):
                sel.append((p, (p + 1) % K))
        fac = run_factors([(s, int(rng.randint(1, 6))) for s in sel], 8, rng)
        out.append(make_case(f"K{K}", K, 8, fac, plain_layout(K, K % 3), 310 + K))
    for n_runs in (7, 8, 9):  # the by-eights gather of the (ext | td)^2 cells, ext and td free
        pairs = [(i, j) for i in range(4) for j in range(4) if i != j][:n_runs]
        fac = run_factors([(s, 2 + k % 3) for k, s in enumerate(pairs)], 6, rng)
        out.append(make_case(f"nruns{n_runs}", 4, 6, fac, plain_layout(4, 0), 320 + n_runs))
    return out


def landmark_row_cases():
    """(case, expected LB or None, minimum LB or None)"""
    rng = np.random.RandomState(400)
    out = []
    # LB = 1: 6 free columns + 1 unowned column per pose, 65 poses -> NB >= 129
    n = 65
    tok = []
    for k in range(n):
        tok += [("pose", k), ("gap", 1)]
    out.append((make_case("LB1", n, 5, spread_factors(n, 5, 2, rng), layout(n, tok + [("ext",), ("td",)]), 401), 1, None))
    # LB = 2: the 6 + 9 interleaving of a visual-inertial window at 33 poses (P = 33 * 15 + 7 = 502)
    n = 33
    tok = []
    for k in range(n):
        tok += [("pose", k), ("gap", 9)]
    out.append((make_case("LB2", n, 5, spread_factors(n, 5, 2, rng), layout(n, tok + [("ext",), ("td",)]), 402), 2, None))
    # LB >= 25, and one landmark with more than ASML_FB factors (landmark 0: 70), so that one thread's walk crosses a staging pass
    fac = spread_factors(6, 30, 8, rng) + [(1 + k % 5, 0, 0) for k in range(35)] + [(0, 1 + k % 5, 0) for k in range(35)]
    fac = [fac[k] for k in rng.permutation(len(fac))]
    out.append((make_case("long_landmark", 6, 30, fac, plain_layout(6, 0), 403), None, 25))
    # gap runs of 1, 6, 7 and 13 columns, a gap at column 0, col_td = 0 is its own case below; a constant pose in the middle
    tok = [("gap", 13), ("pose", 0), ("gap", 1), ("pose", 1), ("gap", 6), ("pose", 3), ("td",), ("gap", 7), ("pose", 4), ("ext",), ("pose", 5)]
    out.append((make_case("gaps", 6, 12, spread_factors(6, 12, 5, rng), layout(6, tok), 404), None, None))
    tok = [("td",), ("pose", 0), ("pose", 1), ("ext",), ("pose", 2), ("pose", 3)]
    out.append((make_case("td_first", 4, 9, spread_factors(4, 9, 4, rng), layout(4, tok), 405), None, None))
    for nm, ext, td in (("no_td", True, False), ("no_ext", False, True), ("no_ext_no_td", False, False)):
        out.append((make_case(nm, 5, 9, spread_factors(5, 9, 4, rng), plain_layout(5, 3, ext=ext, td=td), 406 + len(out)), None, None))
    return out


def clamp_cases():
    """min_diag / max_diag are set by the check body to the 30th and 70th percentile of the reference's positive h_ll"""
    rng = np.random.RandomState(500)
    fac = [f for f in spread_factors(7, 40, 12, rng) if f[2] != 3]
    return [make_case("clamps", 7, 40, fac, plain_layout(7, 2), 501, damps=(0.0, 1e-4, 3.0), clamp_percentiles=(30, 70))]


def clamp_batch():
    rng = np.random.RandomState(510)
    lay = plain_layout(7, 2)
    return [make_case(f"clamp_batch_{k}", 7, L, spread_factors(7, L, 10, rng), lay, 511 + k, clamp_percentiles=(30, 70)) for k, L in enumerate((25, 33))]


def determinism_batch():
    """window 0 has K < Kmax and NB < NBmax in the launch it shares with window 1 (same P = 97: two reduce workgroups, LT 30)"""
    rng = np.random.RandomState(600)
    small = make_case("det_small", 5, 31, spread_factors(5, 31, 12, rng), plain_layout(5, 97 - 37), 601)
    tok = []
    for k in range(12):
        tok += [("pose", k), ("gap", 1)]
    big = make_case("det_big", 12, 20, spread_factors(12, 20, 6, rng), layout(12, tok + [("ext",), ("td",), ("gap", 6)]), 602)
    assert small["P"] == big["P"] == 97
    return [small, big]


def wide_batch():
    """two windows of P = 257: the second accs slot in a launch whose blockIdx.y is not 0"""
    return [_width_case(257, 20, 700), _width_case(257, 9, 701)]


def count_cases():
    """windows of 1, 255, 256, 257 and 513 factors for k_reproj_cost_w (256 threads per window) and k_reproj_chi2 (256 per workgroup)"""
    rng = np.random.RandomState(800)
    out = []
    for n in (1, 255, 256, 257, 513):
        pairs = [(i, j) for i in range(4) for j in range(4) if i != j]
        fac = [(*pairs[int(rng.randint(0, len(pairs)))], int(rng.randint(0, 10))) for _ in range(n)]
        out.append(make_case(f"count{n}", 4, 10, fac, plain_layout(4, 0), 801 + n, pixel_noise=1.5))
    return out
