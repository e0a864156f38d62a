"""Hand-built degenerate systems for the three Levenberg optimisers (PoseOptimization, TranslationOptimization, OptimizeSim3;
DESIGN.md sections 20 - 22 and 24): per optimiser a dictionary of named scenes made from the restatements' own generators by
overwriting fields, each with the control path it is meant to take, and paths(), which runs a restatement with counters hung on
it from outside and says which paths a scene took.  Pure numpy plus the three restatements; nothing of the library is imported.
Used by tests/test_lm_edges_cpu.py and tests/test_gpu_lm_edges.py."""
import math

import numpy as np

import pose_opt_numpy as pn
import sim3_opt_numpy as sn
import trans_opt_numpy as tn

F, D = np.float32, np.float64
OPTIMISERS = ("pose_opt", "trans_opt", "sim3_opt")
MODULE = {"pose_opt": pn, "trans_opt": tn, "sim3_opt": sn}
CHUNK, PLANE_CHUNK, WAVE = 256, 16, 64              # the point / line edges of a pass, k_pose_opt's plane edges of a pass, a wavefront
SIM3_CHUNK = CHUNK // 2                             # k_sim3_opt's pass takes 256 edges, e12 and e21 of 128 matches


# ------------------------------------------------------------------------------------------------------------------------------
# what the device's certificates refuse, from the ranges cr_cube.h, cr_sincos.h and cr_atan2.h document
def cube_uncertifiable(x):
    """"range" outside (2^-300, 2^300), "tie" for an x of at most 18 significant bits whose cube has 54, else None"""
    x = float(x)
    if x != x or math.isinf(x) or x == 0.0:
        return None                                 # pow(v, 3) of these is v * v * v on both sides
    ax = abs(x)
    if not 2.0 ** -300 < ax < 2.0 ** 300:
        return "range"
    m = int(math.frexp(ax)[0] * 2 ** 53)
    m //= m & -m                                    # the odd part of the significand
    if m.bit_length() <= 18 and (m ** 3).bit_length() == 54:
        return "tie"                                # an odd 54-bit cube lies exactly between two doubles
    return None


def sincos_uncertifiable(x):
    x = float(x)
    if x != x or math.isinf(x):
        return None
    return "range" if abs(x) >= 64.0 else None


def atan2_uncertifiable(y, x):
    y, x = abs(float(y)), float(x)
    if y != y or x != x or y == 0 or x == 0 or math.isinf(y) or math.isinf(x):
        return None
    if x > 0 and math.frexp(x)[1] - math.frexp(y)[1] > 62 and y / x < 2.0 ** -1022:
        return "subnormal"
    return None


def pivots(A):
    """The pivot search of Eigen's LDLT alone, on a copy: (the transpositions, smallest |pivot| / largest |pivot|, the diagonal it
    started from)"""
    n = len(A)
    A = np.array(A, D)
    diag = [float(v) for v in np.diag(A)]
    tr, piv = [], []
    with np.errstate(all="ignore"):
        for k in range(n):
            big = k + int(np.argmax(np.abs(np.diag(A)[k:])))
            tr.append(big)
            if big != k:
                A[[k, big]] = A[[big, k]]
                A[:, [k, big]] = A[:, [big, k]]
            piv.append(abs(float(A[k, k])))
            if A[k, k] == 0 or A[k, k] != A[k, k]:
                break
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:]) / A[k, k]
    top = max(piv)
    return tr, (min(piv) / top if top > 0 and math.isfinite(top) else 0.0), diag


def paths(optimiser, scene):
    """Runs the restatement of `optimiser` on `scene` with counters hung on its module functions (ldlt_solve / ldlt_solve7, cr_cube,
    cr_sincos, cr_atan2, oplus) and on Optimizer.optimize / active_chi2 and Graph.huber (for the translation also
    Graph.quadratic_terms), which change no value.  Returns the counts, and the
    restatement's output under "out".  The trial a solve belongs to is the first oplus after it; a cube outside oplus is Levenberg's
    and is taken only by an accepted trial; how an optimize() call stopped follows from its iteration and trial counts:
      solves, failed_solves      LDLT calls, and those that were not isPositive()
      accepted_after_failed      trials kept although their solve failed (rho > 0 through a negative computeScale)
      good_after_failed          iterations in which a failed solve was followed by a good one
      stale_x                    failed solves that left a non-zero x of an earlier solve to the update
      stale_x_across_calls       .. an x written in an earlier optimize() call
      stale_x_after_empty        .. an x written before an optimize() call that had no active edge
      stops                      per optimize() call "empty", "qmax" (ten trials), "nbad", "limit" or "rho0"
      rho0_first_then_more       a call stopped by rho == 0 in its first iteration and a later call iterated
      max_theta                  the largest finite |omega| of a trial's update
      uncertifiable              (function, why, argument, where) of every argument the device would not certify; for the
                                 translation also ("terms", "nonfinite", edges, "build"), k_trans_opt's 0 * inf test
      hand_back                  uncertifiable is not empty
      sigma_nonzero              Sim3: a non-zero log scale reached exp in a trial
      thetas                     |omega| of every trial's update, in order
      huber_at_delta             robust-kernel arguments equal to delta^2 exactly
      first_swaps, first_tr, first_pivot_ratio, first_diag    pivots() of the first system solved"""
    seven = optimiser == "sim3_opt"
    r = dict(solves=0, failed_solves=0, accepted=0, accepted_after_failed=0, good_after_failed=0, stale_x=0, stale_x_across_calls=0,
             stale_x_after_empty=0, stops=[], trials_per_iteration=[], max_theta=0.0, uncertifiable=[], sigma_nonzero=False,
             first_swaps=None, first_pivot_ratio=None, first_tr=None, first_diag=None, thetas=[], huber_at_delta=0)
    st = dict(in_oplus=0, pending=False, chi_of_trial=False, last_ok=None, x_call=-1, call=-1, trials=None, failed=False, its=[],
              empty_since_x=False, me=None, quiet=False)
    solver = (sn, "ldlt_solve7") if seven else (pn, "ldlt_solve")
    upd = sn if seven else pn
    cls = sn.Optimizer if seven else pn.Optimizer
    saved = []

    def hang(owner, name, make):
        old = getattr(owner, name)
        saved.append((owner, name, old))
        setattr(owner, name, make(old))

    def w_solve(old):
        def f(H, b):
            ok, x = old(H, b)
            r["solves"] += 1
            if r["first_swaps"] is None:
                r["first_tr"], r["first_pivot_ratio"], r["first_diag"] = pivots(H)
                r["first_swaps"] = sum(1 for k, big in enumerate(r["first_tr"][:-1]) if big != k)
            if ok:
                st["x_call"], st["empty_since_x"] = st["call"], False
                if st["failed"]:
                    r["good_after_failed"] += 1
                    st["failed"] = False
            else:
                r["failed_solves"] += 1
                st["failed"] = True
                if any(v != 0 for v in st["me"].x):
                    r["stale_x"] += 1
                    r["stale_x_across_calls"] += st["x_call"] != st["call"]
                    r["stale_x_after_empty"] += bool(st["empty_since_x"])
            st["last_ok"], st["pending"], st["chi_of_trial"] = ok, True, True
            st["trials"] += 1
            return ok, x
        return f

    def w_oplus(old):
        def f(*a):
            if st["pending"] and not st["in_oplus"]:
                st["pending"] = False
                u = a[1] if seven else a[2]
                th = pn._sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
                r["thetas"].append(th)
                if math.isfinite(th):
                    r["max_theta"] = max(r["max_theta"], th)
                if seven and u[6] != 0 and not a[2]:
                    r["sigma_nonzero"] = True
            st["in_oplus"] += 1
            try:
                return old(*a)
            finally:
                st["in_oplus"] -= 1
        return f

    def w_cube(old):
        def f(x):
            why = cube_uncertifiable(x)
            if why:
                r["uncertifiable"].append(("cube", why, float(x), "exp" if st["in_oplus"] else "levenberg"))
            if not st["in_oplus"]:
                r["accepted"] += 1
                r["accepted_after_failed"] += st["last_ok"] is False
            return old(x)
        return f

    def w_sincos(old):
        def f(t):
            why = sincos_uncertifiable(t)
            if why:
                r["uncertifiable"].append(("sincos", why, float(t), "exp" if st["in_oplus"] else "plane"))
            return old(t)
        return f

    def w_atan2(old):
        def f(y, x):
            why = atan2_uncertifiable(y, x)
            if why:
                r["uncertifiable"].append(("atan2", why, (float(y), float(x)), "plane"))
            return old(y, x)
        return f

    def w_chi(old):
        def f(self, *a):
            if not st["chi_of_trial"]:              # the call no solve precedes opens an iteration
                if st["trials"] is not None:
                    st["its"].append(st["trials"])
                st["trials"], st["failed"] = 0, False
            st["chi_of_trial"] = False
            return old(self, *a)
        return f

    def w_optimize(old):
        def f(self, *a, **kw):
            st["me"] = self
            st["call"] += 1
            st["its"], st["trials"], st["chi_of_trial"] = [], None, False
            nb0, it0 = self.nbad_stops, self.iterations
            limit = a[1] if seven else (a[2] if len(a) > 2 else kw.get("its", 10))
            out = old(self, *a, **kw)
            if st["trials"] is not None:
                st["its"].append(st["trials"])
            n_it = self.iterations - it0
            assert n_it == len(st["its"])
            r["trials_per_iteration"].append(list(st["its"]))
            if n_it == 0:
                why = "empty"
                st["empty_since_x"] = True
            elif st["its"][-1] == 10:
                why = "qmax"
            elif self.nbad_stops > nb0:
                why = "nbad"
            elif n_it == limit:
                why = "limit"
            else:
                why = "rho0"
            r["stops"].append(why)
            return out
        return f

    def w_huber(old):
        def f(self, *a):
            c = a[-1]
            dsqr = float(D(F(self.delta * self.delta))) if seven else self.dsqr[a[0]]
            if not st["quiet"]:
                r["huber_at_delta"] += int(np.sum(np.asarray(c) == dsqr))
            return old(self, *a)
        return f

    def w_terms(old):
        def f(self, idx, J, e, robust):
            # k_trans_opt leaves the rotation rows and columns out and hands a frame back when one of them would not be +-0:
            # a factor of a zero column (the error, rho1 Omega, A^T W, a translation column) that is not finite
            with np.errstate(all="ignore"):
                st["quiet"] = True
                rho1 = self.huber(idx, self.chi2(idx, e))[1] if robust else np.ones(len(idx))
                st["quiet"] = False
                used = np.arange(3)[None, :] < self.dim[idx][:, None]
                w = rho1[:, None] * self.info[idx]
                A = J[:, :, 3:]
                fin = np.isfinite(rho1)[:, None] & np.isfinite(e) & np.isfinite(w) & np.isfinite(A).all(axis=2)
                fin &= np.isfinite(A * w[:, :, None]).all(axis=2)
                fin &= np.isfinite((rho1[:, None, None] * A) * self.info[idx][:, :, None]).all(axis=2)
                bad = int((~fin & used).any(axis=1).sum())
            if bad:
                r["uncertifiable"].append(("terms", "nonfinite", bad, "build"))
            return old(self, idx, J, e, robust)
        return f

    if optimiser == "trans_opt":
        hang(pn.Graph, "quadratic_terms", w_terms)
    hang(sn.Graph if seven else pn.Graph, "huber", w_huber)
    hang(solver[0], solver[1], w_solve)
    hang(upd, "oplus", w_oplus)
    hang(pn, "cr_cube", w_cube)
    hang(pn, "cr_sincos", w_sincos)
    hang(pn, "cr_atan2", w_atan2)
    hang(cls, "optimize", w_optimize)
    hang(cls, "active_chi2", w_chi)
    try:
        run = {"pose_opt": pn.pose_optimization, "trans_opt": tn.translation_optimization, "sim3_opt": sn.optimize_sim3}[optimiser]
        r["out"] = run(scene)
    finally:
        for owner, name, old in reversed(saved):
            setattr(owner, name, old)
    r["rho0_first_then_more"] = any(why == "rho0" and len(r["trials_per_iteration"][i]) == 1 and
                                    any(w != "empty" for w in r["stops"][i + 1:]) for i, why in enumerate(r["stops"]))
    r["rho0_stops"], r["qmax_stops"] = r["stops"].count("rho0"), r["stops"].count("qmax")
    r["hand_back"] = bool(r["uncertifiable"])
    return r


_PATHS = {}


def scene_paths(optimiser, name):
    """paths() of a named scene, computed once per process"""
    if (optimiser, name) not in _PATHS:
        _PATHS[optimiser, name] = paths(optimiser, scenes(optimiser)[name]["scene"])
    return _PATHS[optimiser, name]


# ------------------------------------------------------------------------------------------------------------------------------
# the scenes.  A scene is dict(scene=<what the generator makes>, path=<one line>, expect=<what paths() must report>); expect holds
# minimum counts under paths()' names, and "stops" / "first_swaps" / "first_tr" / "hand_back" / "flags" exactly.  Seeds were found by
# searching the restatement; tests/test_lm_edges_cpu.py holds every scene to its expectation.
_rs = np.random.default_rng
EXACT_K = (512.0, 512.0, 320.0, 240.0)              # projections of dyadic points are exact floats
TH_MONO, TH_STEREO, TH_LINE = F(5.991), F(7.815), F(2) * F(5.991)


def _cp(f):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()}


def _neg(f, keys, sel=slice(None), factor=-1.0):
    f = _cp(f)
    for k in keys:
        f[k][sel] = (f[k][sel] * F(factor)).astype(F)
    return f


def _near(v):
    """the float below, v itself, the float above"""
    v = F(v)
    return np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))


def _delta_sq(th):
    """float dsqr = delta * delta of the Huber kernel whose delta is (float)sqrt(th)"""
    d = D(F(math.sqrt(th)))
    return F(d * d)


def _frame_threshold_scene(gen):
    """The identity pose, K exact.  Every edge sits on the optical axis at depth 2 and comes with a twin whose error is the
    negative: b is zero to the bit, the first solve returns x = 0, rho is 0 and the pose never moves, so the classification sees the
    errors as they are built here.  Pairs of mono points, stereo points and lines whose chi2 is the float below the threshold, the
    threshold and the float above: only the last of each kind is an outlier."""
    fx, fy, cx, cy = EXACT_K
    obs, ur, w, Xw, flags = [], [], [], [], []
    for th, stereo in ((TH_MONO, False), (TH_STEREO, True)):
        for i, t in enumerate(_near(th)):
            for sign in (1.0, -1.0):
                obs.append((cx + 2.0 * sign, cy))                  # e = (+-2, 0): chi2 = 2 * (w * 2) = 4 w = t
                ur.append(cx - 40.0 * 0.5 if stereo else -1.0)     # bf / z = 20: the third error is zero
                w.append(t / F(4))
                Xw.append((0.0, 0.0, 2.0))
                flags.append(int(i == 2))
    fn, ends, lflags = [], [], []
    for i, t in enumerate(_near(TH_LINE)):
        e = float(D(3.0 * cx - 4.0 * cy) + D(-(3.0 * cx - 4.0 * cy) + math.sqrt(float(t))))        # exact: the line is (3, -4, c)
        assert F(e * e) == t
        for sign in (1.0, -1.0):
            fn.append((3.0, -4.0, -(3.0 * cx - 4.0 * cy) + sign * e))
            ends.append((0.0, 0.0, 2.0, 0.0, 0.0, 2.0))
            lflags.append(int(i == 2))
    fr = gen(_rs(0), len(obs), len(fn), identity=True, K=EXACT_K)
    fr.update(obs=np.array(obs, F), u_right=np.array(ur, F), inv_sigma2=np.array(w, F), Xw=np.array(Xw, F),
              line_fn=np.array(fn, D), line_ends=np.array(ends, D), Tcw=np.eye(4, dtype=F).reshape(16))
    return fr, dict(point_outlier=flags, line_outlier=lflags)


def _frame_huber_scene(gen, seed):
    """A planted frame at the identity whose first six points sit on the optical axis with the error (1, 0): their chi2 is their
    information, set to the float below delta^2, delta^2 and the float above, mono and stereo.  The frame moves, so the branch
    Huber takes for them shows in every bit of the result."""
    fr = gen(_rs(seed), 14, identity=True)
    cx, cy = (float(D(F(v))) for v in pn.CAM[2:])
    for i in range(6):
        stereo = i % 2 == 1                                         # frame() makes the odd points stereo
        fr["Xw"][i] = (0.0, 0.0, 2.0)
        fr["obs"][i] = (F(cx) + F(1), F(cy))
        fr["u_right"][i] = F(cx - float(D(F(pn.BF))) * 0.5) if stereo else F(-1)
        fr["inv_sigma2"][i] = _near(_delta_sq(7.815 if stereo else 5.991))[i // 2]
    return fr


def _first_step(fr):
    """|omega| of the first trial's update of a pose frame, through the restatement's own pieces"""
    o = pn.Optimizer(fr)
    g = o.g
    act = np.nonzero(~g.level)[0]
    q, t = pn.to_se3quat(fr["Tcw"])
    o.active_chi2(act, q, t)
    Ht, bt = g.quadratic_terms(act, g.jacobians(act, q, t), g.err[act], True)
    H, b = pn.ordered_sum(Ht), pn.ordered_sum(-bt)
    lam = 1e-5 * max(abs(float(H[j, j])) for j in range(6))
    ok, x = pn.ldlt_solve([[float(H[i, j]) + (lam if i == j else 0.0) for j in range(6)] for i in range(6)], [float(v) for v in b])
    assert ok
    return pn._sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])


def _theta_scenes():
    """Two pose frames whose first update has |omega| on either side of SE3Quat::exp's 1e-5: twin points on a dyadic grid (b gets
    nothing from them, H is well conditioned) and one line through the optical axis whose offset alone drives the step; the offset,
    a double, is bisected on its bits until the two neighbouring offsets straddle the threshold."""
    fx, fy, cx, cy = EXACT_K
    obs, Xw = [], []
    for z in (2.0, 4.0):
        for x in (-1.0, 0.0, 1.0):
            for y in (-0.5, 0.5):
                for sign in (1.0, -1.0):
                    obs.append((cx + fx * x / z + sign, cy + fy * y / z + 0.5 * sign))
                    Xw.append((x, y, z))
    base = pn.frame(_rs(0), len(obs), 1, identity=True, K=EXACT_K, mode="mono")
    base.update(obs=np.array(obs, F), inv_sigma2=np.ones(len(obs), F), Xw=np.array(Xw, F), Tcw=np.eye(4, dtype=F).reshape(16),
                line_ends=np.array([[0.0, 0.0, 2.0, 0.0, 0.0, 4.0]], D))

    def at(bits):
        fr = _cp(base)
        fr["line_fn"] = np.array([[3.0, -4.0, -(3.0 * cx - 4.0 * cy) + float(np.int64(bits).view(D))]], D)
        return fr
    # the offset and the line error are the same number only while 3 cx - 4 cy cancels exactly
    assert 3.0 * cx - 4.0 * cy == 0.0
    lo, hi = np.float64(1e-9).view(np.int64), np.float64(1.0).view(np.int64)
    assert _first_step(at(lo)) < 1e-5 <= _first_step(at(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _first_step(at(mid)) < 1e-5:
            lo = mid
        else:
            hi = mid
    return at(lo), at(hi)


def _frame_scenes(optimiser):
    pose = optimiser == "pose_opt"
    gen = pn.frame if pose else tn.tframe
    I = ("inv_sigma2",)
    S = {}

    def add(name, scene, path, **expect):
        expect.setdefault("hand_back", False)
        S[name] = dict(scene=scene, path=path, expect=expect)
    # 1. the zero system
    f = gen(_rs(0), 12)
    f["inv_sigma2"][:] = 0
    add("zero_system", f, "H = 0, lambda = 0, a zero first pivot, x = 0: rho == 0 stops iteration 0 of all four rounds",
        stops=["rho0"] * 4, rho0_first_then_more=1)
    f = gen(_rs(0), 24, outlier_frac=0.3, outlier_px=(150, 300), mode="stereo")
    f["inv_sigma2"][~f["planted_outlier"]] = 0
    add("zero_later", f, "only the planted outliers carry information: once they are flagged the rounds that follow are zero systems",
        stops=["nbad", "nbad", "rho0", "rho0"] if pose else ["nbad", "rho0", "rho0", "rho0"], rho0_first_then_more=1)
    # 2. negative information: failed solves, kept trials after a failed solve, Levenberg's cube far out of range (scene 8), and
    # 5. a failed first solve of a round that reads the x of the round before
    neg = dict(failed_solves=1, accepted_after_failed=1, good_after_failed=1, stale_x_across_calls=1, hand_back=True, cube_range=1)
    add("negative_mono", _neg(gen(_rs(0), 12, mode="mono"), I), "every solve with a small lambda fails; tempChi = DBL_MAX is accepted",
        **neg)
    add("negative_stereo", _neg(gen(_rs(0 if pose else 1), 12, mode="stereo"), I), "as negative_mono, three-dimensional edges", **neg)
    add("negative_lines_plane", _neg(gen(_rs(0 if pose else 1), 12, 2, planes=(pn.MATCHED,)), I),
        "as negative_mono with two lines and a plane slot, whose information stays positive", **neg)
    add("negative_rejected", _neg(gen(_rs(1 if pose else 4), 12, mode="mono"), I),
        "negative information and no failed solve accepted: nothing is handed back, the rows are the device's own",
        failed_solves=1, good_after_failed=1, stale_x_across_calls=1, accepted_after_failed_exactly=0)
    # 3. mixed sign
    add("mixed_sign", _neg(gen(_rs(0 if pose else 11), 12), I, slice(0, None, 2)),
        "H + lambda I is indefinite until lambda has doubled often enough: a failed solve, then a good one, in one iteration" +
        ("" if pose else "; failed solves are accepted with a cube inside the certified range, so the frame stays on the device"),
        failed_solves=1, good_after_failed=1, **({} if pose else dict(accepted_after_failed=1)))
    # 4. ten rejected trials
    add("qmax_negative", _neg(gen(_rs(39), 12, mode="mono") if pose else gen(_rs(8), 12, mode="stereo"), I),
        "negative information: ten trials of one iteration are rejected", qmax_stops=1, failed_solves=1, hand_back=not pose)
    add("qmax_far_start", gen(_rs(6), 30, start_trans=3.0, start_rot=0.8, noise=0.1) if pose else
        gen(_rs(3), 30, start_trans=3.0, noise=0.1),
        "every solve succeeds, the start is far outside the basin and every step raises the chi2: qmax == 10 with a finite negative rho",
        qmax_stops=1, failed_solves_exactly=0)
    # 6. rank deficiency without a sign error
    f = gen(_rs(3), 12)
    f["Xw"][:] = f["Xw"][0]
    add("coincident_points", f, "all map points coincide", pivot_ratio_below=2e-5, failed_solves_exactly=0)
    f = gen(_rs(4), 12, mode="mono", identity=True)
    f["Xw"][:, :2] = 0
    add("points_on_axis", f, "all map points on the optical axis, mono", pivot_ratio_below=2e-5, failed_solves_exactly=0)
    add("three_mono_points", gen(_rs(5), 3, mode="mono"), "exactly three mono points: six equations, one round",
        failed_solves_exactly=0, stops=["limit"] if pose else ["nbad"])
    f = gen(_rs(6), 0 if pose else 3, 0, planes=(pn.MATCHED,) * 4, mode="mono")
    f["plane_world"][:, :3] = f["plane_world"][0, :3]
    f["plane_meas"][:, :3] = f["plane_meas"][0, :3]
    add("parallel_planes", f, "four planes with one normal" + ("" if pose else " beside the three points the function asks for"),
        pivot_ratio_below=2e-5, failed_solves_exactly=0)
    # 7. the permutation of Eigen::LDLT
    if pose:
        f = gen(_rs(7), 12, mode="mono", identity=True, K=(300.0, 900.0, 320.0, 240.0))
        f["Xw"] = (f["Xw"] * F(0.01)).astype(F)
        add("ldlt_every_step_swaps", f, "depth / 100: the translation rows outweigh the rotation rows", first_swaps=5)
        add("ldlt_no_swap", gen(_rs(7), 12, mode="mono", identity=True), "the first system's pivots come in order", first_swaps=0)
    else:
        # the rotation rows of H are zero: their pivots are lambda and the three translation rows always come first
        f = gen(_rs(7), 12, mode="mono", identity=True, K=(300.0, 900.0, 320.0, 240.0))
        add("ldlt_y_first", f, "fy > fx: the y row is the first pivot", first_tr=[4, 3, 5, 3, 4, 5])
        f = gen(_rs(7), 12, mode="mono", identity=True, K=(900.0, 300.0, 320.0, 240.0))
        add("ldlt_x_first", f, "fx > fy: the x row is the first pivot", first_tr=[3, 4, 5, 3, 4, 5])
    # 8. an update the device's sin / cos cannot certify
    if pose:
        add("theta_above_64", _neg(gen(_rs(2), 12, mode="mono"), I), "negative information, a near-singular solve: an update angle of 118.9",
            max_theta=64.0, sincos_range=1, hand_back=True)
    # 9. thresholds
    f, flags = _frame_threshold_scene(gen)
    add("chi2_at_thresholds", f, "chi2 one float below, at and one float above 5.991f / 7.815f / 2 * 5.991f at the classification",
        stops=["rho0"] * 4, flags=flags)
    add("huber_at_delta", _frame_huber_scene(gen, 11), "Huber's argument one float below, at and above delta^2 in the first pass",
        huber_at_delta=2)
    if pose:
        lo, hi = _theta_scenes()
        add("theta_below_1e-5", lo, "the first update's angle is the largest this scene reaches below 1e-5",
            first_theta_below=(1e-5, 1e-14))
        add("theta_at_1e-5", hi, "the next offset: the angle is 1e-5 or just above", first_theta_from=(1e-5, 1e-14))
    # 10. seams: the one edge of negative information at either side of a chunk's end.  Seed and weight are chosen so that no failed
    # solve is accepted: the frame is not handed back and the rows compared are the device's own
    for k, (seed, w) in zip((CHUNK - 2, CHUNK - 1, CHUNK), ((20, -10.0), (20, -10.0), (21, -100.0)) if pose else ((36, -3000.0),) * 3):
        f = gen(_rs(seed), CHUNK + 1, noise=0.3)
        f["inv_sigma2"][k] = F(w)
        add(f"seam_point_{k}", f, f"257 points, edge {k} alone has negative information, large enough to make H indefinite",
            failed_solves=1, good_after_failed=1)
    add("negative_257", _neg(gen(_rs(40 if pose else 41), CHUNK + 1, noise=0.3), I),
        "257 points, all of negative information, no failed solve accepted: two chunks of the device's own rows",
        failed_solves=1, good_after_failed=1, stale_x_across_calls=1, accepted_after_failed_exactly=0)
    for j, (seed, sel) in zip((PLANE_CHUNK - 1, PLANE_CHUNK), ((23, slice(None)), (23, slice(0, None, 3))) if pose else
                              ((24, slice(None)), (23, slice(None)))):
        f = _neg(gen(_rs(seed), 12, planes=(pn.MATCHED,) * (PLANE_CHUNK + 1)), I, sel)
        f["plane_meas"][j] = f["plane_meas"][j][[1, 2, 0, 3]] * np.array([1, -1, 1, 1], F) + np.array([0, 0, 0, 2.0], F)
        add(f"seam_plane_{j}", f, f"negative points and 17 plane edges, plane edge {j} alone measured wrongly", failed_solves=1)
    return S


def _sim3_twin_scene():
    """The identity, both cameras alike, every point on both optical axes: match 2j + 1 is match 2j with the negative error, so b is
    zero, the step is zero and rho == 0 ends both optimize() calls before the estimate moves.  chi2 = 4 w of one edge of a pair is
    the float below th2 = 10, th2 and the float above, for e12 and for e21; six more pairs are plain inliers."""
    pr = sn.problem(_rs(0), n=24, identity=True)
    cx, cy = (float(D(F(v))) for v in sn.CAM1[2:])
    pr["P3D1w"][:] = (0.0, 0.0, 2.0)
    pr["P3D2w"][:] = (0.0, 0.0, 2.0)
    pr["obs1"][:] = (F(cx), F(cy))
    pr["obs2"][:] = (F(cx), F(cy))
    pr["inv_sigma2_1"][:] = 1
    pr["inv_sigma2_2"][:] = 1
    flags = np.zeros(24, np.uint8)
    m = 0
    for key, wkey in (("obs1", "inv_sigma2_1"), ("obs2", "inv_sigma2_2")):
        for i, w in enumerate(_near(2.5)):                          # 2 * (w * 2) = 4 w: 10 exactly at w = 2.5
            for sign in (1.0, -1.0):
                pr[key][m, 0] = F(cx) + F(2.0 * sign)
                pr[wkey][m] = w
                flags[m] = i == 2
                m += 1
    for j in range(6):
        for sign in (1.0, -1.0):
            pr["obs1"][m, 0] = F(cx) + F(0.25 * (j + 1) * sign)
            m += 1
    return pr, dict(outlier=[int(v) for v in flags])


def _sim3_huber_scene(seed):
    pr = sn.problem(_rs(seed), n=24, identity=True)
    cx, cy = (float(D(F(v))) for v in sn.CAM1[2:])
    d = D(np.sqrt(F(10.0)))
    for i, w in enumerate(_near(F(d * d))):
        pr["P3D1w"][i] = pr["P3D2w"][i] = (0.0, 0.0, 2.0)
        pr["obs1"][i] = (F(cx) + F(1), F(cy))
        pr["obs2"][i] = (F(cx), F(cy))
        pr["inv_sigma2_1"][i] = w
    return pr


def _sim3_first_step(pr):
    """|omega| of the first trial's update of a Sim3 problem, through the restatement's own pieces"""
    o = sn.Optimizer(pr)
    g = o.g
    act = np.nonzero(~g.gone)[0]
    S = sn.s12_tuple(pr["S12"])
    o.active_chi2(act, S)
    sums = sn.ordered_sum(g.terms(act, S, o.fix))
    H = [[float(sums[max(i, j) * (max(i, j) + 1) // 2 + min(i, j)]) for j in range(7)] for i in range(7)]
    lam = 1e-5 * max(abs(H[j][j]) for j in range(7))
    ok, x = sn.ldlt_solve7([[H[i][j] + (lam if i == j else 0.0) for j in range(7)] for i in range(7)], [float(v) for v in sums[28:]])
    assert ok
    return pn._sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])


def _sim3_theta_scenes():
    """Two Sim3 problems without noise at the identity whose start estimate is turned about the optical axis by an angle, a double,
    bisected on its bits until the first update's |omega| straddles Sim3's 1e-5"""
    base = sn.problem(_rs(12), n=24, identity=True, noise=0.0)

    def at(bits):
        a = float(np.int64(bits).view(D))
        pr = _cp(base)
        pr["S12"] = np.array([0.0, 0.0, math.sin(0.5 * a), math.cos(0.5 * a), 0.0, 0.0, 0.0, 1.0], D)
        return pr
    lo, hi = np.float64(1e-7).view(np.int64), np.float64(1e-3).view(np.int64)
    assert _sim3_first_step(at(lo)) < 1e-5 <= _sim3_first_step(at(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _sim3_first_step(at(mid)) < 1e-5:
            lo = mid
        else:
            hi = mid
    return at(lo), at(hi)


def _swap_xy(pr):
    """the scene mirrored in the diagonal of both images: the wide axis of the point cloud becomes y"""
    pr = _cp(pr)
    for k, o, K in (("P3D1w", "obs1", "K1"), ("P3D2w", "obs2", "K2")):
        pr[k] = pr[k][:, [1, 0, 2]].copy()
        fx, fy, cx, cy = (float(v) for v in pr[K])
        u, v = pr[o][:, 0].astype(D), pr[o][:, 1].astype(D)
        pr[o] = np.stack([(v - cy) / fy * fx + cx, (u - cx) / fx * fy + cy], 1).astype(F)
    return pr


def _drawn_sim3(seed):
    """the problem the search over random degenerate problems drew under `seed`: the generator's parameters come from the same
    stream as the problem, in this order"""
    rng = _rs(seed)
    kind = int(rng.integers(0, 5))
    n = int(rng.integers(12, 40))
    fix = 1 if rng.random() < 0.8 else 0
    pr = sn.problem(rng, n=n, fix_scale=fix, outlier_frac=float(rng.choice([0, 0.3, 1.0])),
                    start=(float(rng.choice([0.01, 0.5])), float(rng.choice([0.03, 3.0])), 0.0), far=float(rng.choice([1.0, 1.0, 100.0, 0.01])))
    return kind, pr


def _sim3_scenes():
    I = ("inv_sigma2_1", "inv_sigma2_2")
    S = {}

    def add(name, scene, path, **expect):
        expect.setdefault("hand_back", False)
        S[name] = dict(scene=scene, path=path, expect=expect)
    pr = sn.problem(_rs(0), n=24)
    pr["inv_sigma2_1"][:] = 0
    pr["inv_sigma2_2"][:] = 0
    add("zero_system", pr, "H = 0: rho == 0 stops iteration 0 of both optimize() calls", stops=["rho0", "rho0"], rho0_first_then_more=1)
    pr = sn.problem(_rs(0), n=30)
    rng = _rs(1000)
    pr["obs1"][:8] += (rng.uniform(40, 90, (8, 2)) * rng.choice([-1, 1], (8, 2))).astype(F)
    pr["inv_sigma2_1"][8:] = 0
    pr["inv_sigma2_2"][8:] = 0
    add("zero_later", pr, "only eight gross outliers carry information: the second optimize() is a zero system", stops=["limit", "rho0"])
    neg = dict(failed_solves=1, accepted_after_failed=1, good_after_failed=1, stale_x_across_calls=1, hand_back=True, cube_range=1)
    add("negative", _neg(sn.problem(_rs(16), n=24), I), "negative information, fixed scale: failed solves, one of them accepted, the "
        "second optimize() fails its first solve and steps by the x of the first", **neg)
    add("negative_free_scale", _neg(sn.problem(_rs(10), n=24, fix_scale=0, start=(0.01, 0.03, 0.01)), I),
        "the same with a free scale: sigma != 0 reaches exp; the device hands free-scale problems to the host core", sigma_nonzero=1,
        **neg)
    add("negative_rejected", _neg(sn.problem(_rs(0), n=24), I), "negative information and no failed solve accepted: nothing is handed "
        "back, the rows are the device's own", failed_solves=1, good_after_failed=1, stale_x_across_calls=1,
        accepted_after_failed_exactly=0)
    add("mixed_sign", _neg(sn.problem(_rs(2), n=24), I, slice(0, None, 2)), "every second match negative: a failed solve, then a good "
        "one, in one iteration", failed_solves=1, good_after_failed=1, stale_x_across_calls=1)
    add("qmax_negative", _neg(sn.problem(_rs(40), n=24), I[:1]), "the e12 edges negative: ten rejected trials in the first optimize()",
        qmax_stops=1, failed_solves=1)
    add("qmax_far_start", sn.problem(_rs(20), n=30, start=(0.9, 3.0, 0.0), noise=0.1),
        "every solve succeeds, every step raises the chi2", qmax_stops=1, failed_solves_exactly=0)
    kind, pr = _drawn_sim3(101029)
    assert kind == 4 and pr["fix_scale"] == 1                      # information as generated: nothing is negated
    add("theta_above_64", pr, "positive information, a start far off and a shrunk scene: a near-singular solve steps by an angle of 76",
        max_theta=64.0, sincos_range=1, hand_back=True, failed_solves_exactly=0)
    pr = sn.problem(_rs(3), n=24)
    pr["P3D1w"][:] = pr["P3D1w"][0]
    pr["P3D2w"][:] = pr["P3D2w"][0]
    add("coincident_points", pr, "all map points coincide", pivot_ratio_below=2e-5, failed_solves_exactly=0)
    pr = sn.problem(_rs(4), n=24, identity=True)
    pr["P3D1w"][:, :2] = 0
    pr["P3D2w"][:, :2] = 0
    add("points_on_axis", pr, "all map points on both optical axes", pivot_ratio_below=2e-5, failed_solves_exactly=0)
    add("three_matches", sn.problem(_rs(5), n=3), "three matches: the early return after the first optimize()", failed_solves_exactly=0)
    add("ldlt_every_step_swaps", sn.problem(_rs(4), n=24, far=0.003, K2=(900.0, 300.0, 320.0, 240.0), fix_scale=0, start=(0.01, 0.03, 0.01)),
        "free scale, the scene shrunk to 0.003: translation and scale rows outweigh the rotation rows", first_swaps=6, sigma_nonzero=1)
    add("ldlt_sorted_diagonal", _swap_xy(sn.problem(_rs(0), n=24, far=3.0, identity=True)),
        "the first system's diagonal is already in order: no swap until elimination reorders the rest", diagonal_sorted=1)
    pr, flags = _sim3_twin_scene()
    add("chi2_at_th2", pr, "chi2 one float's worth below, at and above th2 at the classification, for e12 and e21",
        stops=["rho0", "rho0"], flags=flags)
    add("huber_at_delta", _sim3_huber_scene(11), "Huber's argument below, at and above delta^2 in the first pass", huber_at_delta=1)
    lo, hi = _sim3_theta_scenes()
    # the errors pass through products of a few hundred pixels: the angle moves in steps of 1e-13, not of an ulp
    add("theta_below_1e-5", lo, "the first update's angle is the largest this scene reaches below 1e-5", first_theta_below=(1e-5, 1e-7))
    add("theta_at_1e-5", hi, "the next start angle: the update's angle is 1e-5 or just above", first_theta_from=(1e-5, 1e-7))
    # a chunk of k_sim3_opt is 256 edges, 128 matches: the odd match is the last but one of the first chunk, its last, and the one
    # match of the second
    for k in (SIM3_CHUNK - 2, SIM3_CHUNK - 1, SIM3_CHUNK):
        pr = sn.problem(_rs(20), n=SIM3_CHUNK + 1, noise=0.3)
        pr["inv_sigma2_1"][k] = pr["inv_sigma2_2"][k] = F(-100.0)
        add(f"seam_match_{k}", pr, f"129 matches, match {k} alone has negative information", failed_solves=1, good_after_failed=1)
    add("negative_129", _neg(sn.problem(_rs(42), n=SIM3_CHUNK + 1, noise=0.3), I),
        "129 matches, all of negative information, no failed solve accepted: two chunks of the device's own rows",
        failed_solves=1, good_after_failed=1, stale_x_across_calls=1, accepted_after_failed_exactly=0)
    return S


_SCENES = {}


def scenes(optimiser):
    """name -> dict(scene, path, expect) of `optimiser`, built once per process and never modified"""
    if optimiser not in _SCENES:
        _SCENES[optimiser] = _sim3_scenes() if optimiser == "sim3_opt" else _frame_scenes(optimiser)
    return _SCENES[optimiser]


def unmet(r, expect):
    """the entries of a scene's expectation that paths()' result r does not meet"""
    bad = []
    for k, v in expect.items():
        if k == "flags":
            got = {n: [int(x) for x in r["out"][n]] for n in v}
            ok = got == v
        elif k in ("stops", "first_swaps", "first_tr", "hand_back"):
            ok = r[k] == v
        elif k.endswith("_exactly"):
            ok = r[k[:-8]] == v
        elif k == "cube_range":
            ok = sum(u[:2] == ("cube", "range") for u in r["uncertifiable"]) >= v
        elif k == "sincos_range":
            ok = sum(u[:2] == ("sincos", "range") for u in r["uncertifiable"]) >= v
        elif k == "pivot_ratio_below":
            ok = r["first_pivot_ratio"] < v
        elif k == "diagonal_sorted":
            d = r["first_diag"]
            ok = all(d[i] > d[i + 1] for i in range(len(d) - 1))
        elif k == "first_theta_below":                              # v = (threshold, how near, relatively)
            ok = v[0] * (1 - v[1]) <= r["thetas"][0] < v[0]
        elif k == "first_theta_from":
            ok = v[0] <= r["thetas"][0] < v[0] * (1 + v[1])
        else:
            ok = r[k] >= v
        if not ok:
            bad.append(k)
    return bad


def hand_backs(optimiser, names):
    """how many of the named scenes the device must hand back: those with an argument its certificates refuse, counted by paths().
    A Sim3 problem with a free scale never reaches the device and is counted as free_scale, not as handed back."""
    n = 0
    for name in names:
        sc = scenes(optimiser)[name]["scene"]
        if optimiser == "sim3_opt" and not sc["fix_scale"]:
            continue
        n += scene_paths(optimiser, name)["hand_back"]
    return n


_PLAIN = {}


def plain(optimiser, seed, n=12):
    """a plain planted scene to stand beside the edge scenes in a call; one object per (optimiser, seed, n)"""
    key = (optimiser, seed, n)
    if key not in _PLAIN:
        if optimiser == "sim3_opt":
            _PLAIN[key] = sn.problem(_rs(seed), n=2 * n)
        else:
            _PLAIN[key] = (pn.frame if optimiser == "pose_opt" else tn.tframe)(_rs(seed), n, 1 if seed % 3 == 0 else 0)
    return _PLAIN[key]


def interleaved(optimiser, names, order="listed"):
    """[(name or None, scene)]: the named scenes with a plain scene after each, as listed, reversed or sorted by trial count"""
    names = list(names)
    if order == "reversed":
        names.reverse()
    elif order == "by_trials":
        names.sort(key=lambda n: scene_paths(optimiser, n)["solves"])
    items = []
    for k, n in enumerate(names):
        items.append((n, scenes(optimiser)[n]["scene"]))
        items.append((None, plain(optimiser, 500 + k % 7)))
    return items


_PLAIN_OUT = {}


def _out(optimiser, name, scene):
    if name is not None:
        return scene_paths(optimiser, name)["out"]
    key = (optimiser, id(scene))
    if key not in _PLAIN_OUT:
        run = {"pose_opt": pn.pose_optimization, "trans_opt": tn.translation_optimization, "sim3_opt": sn.optimize_sim3}[optimiser]
        _PLAIN_OUT[key] = (scene, run(scene))
    return _PLAIN_OUT[key][1]


def expected_table_of(optimiser, items):
    """the restatement's table of a call over `items` ([(name or None, scene)]), from outputs computed once per scene"""
    m = MODULE[optimiser]
    outs = [_out(optimiser, n, s) for n, s in items]
    run = {"pose_opt": "pose_optimization", "trans_opt": "translation_optimization", "sim3_opt": "optimize_sim3"}[optimiser]
    old = getattr(m, run)
    it = iter(outs)
    setattr(m, run, lambda scene: next(it))
    try:
        return m.table([s for _, s in items])
    finally:
        setattr(m, run, old)


def expected_table(optimiser, names):
    return expected_table_of(optimiser, [(n, scenes(optimiser)[n]["scene"]) for n in names])
