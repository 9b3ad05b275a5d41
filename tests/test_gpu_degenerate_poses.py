"""The distance, clearance, near-pair and witness kernels (mjpl_amd/csrc/mjpl_distance.h, mjpl_distance_grad.h) at
the poses where they branch: the touching, aligned and coincident families of tests/degenerate_cases.py, run through
the pod models of tests/pose_pods.py.  Expected values: the longdouble statement of tests/narrowphase_cases.py on the
target pair where its cores are apart, the NumPy statement of tests/distance_reference.py elsewhere, both at the CPU
oracle's poses.  The bounds are those of tests/test_gpu_distance.py, test_gpu_clearance_grad.py and
test_gpu_near_pairs.py; tests/test_degenerate_cases_host.py checks the sets and the two statements without a GPU."""
import numpy as np
import pytest

import degenerate_cases as dc
import distance_reference as ref
import gradient_reference as gref
import narrowphase_cases as nc
import pose_pods as pods
from mjpl_amd import engine as eng_mod
from mjpl_amd.constraint.collision_constraint import contact_hits
from test_gpu_distance import TOL

pytestmark = pytest.mark.gpu

INF = float("inf")
LD = nc.LD
WITNESS_TOL = 1e-9   # witnesses on their geoms, w2 - w1 = D n, the gradient: test_gpu_near_pairs.test_against_numpy
UNIT_TOL = 1e-12     # |n| = 1
CLOSED_TOL = 1e-12   # closed forms: test_gpu_distance.test_known_answers
STEP = 1e-8          # item 6: the separating translation, a little longer and a little shorter
PUSH_STATUS_UNMOVED = (eng_mod.PUSH_STUCK, eng_mod.PUSH_DEGENERATE)  # tests/test_gpu_push_out.py: check_abc


def run_engine(name):
    """Everything the kernels say about the set, through a fresh engine"""
    cs, m = dc.case_set(name), dc.model_of(name)
    Q = np.ascontiguousarray(cs["Q"])
    e = eng_mod.Engine(m)
    pairs, ia, ib = pods.pair_table(e, m)
    P = len(pairs)
    out = dict(pairs=pairs, ia=ia, ib=ib, D=e.distances(Q), hits=contact_hits(e.contacts(Q), P), clear=e.clearance(Q),
               near=e.near_pairs(Q, INF, max_pairs=P), cgrad=e.clearance_grad(Q))
    e.close()
    return out


def _where(cs, i, pair):
    cls = int(cs["cls"][i])
    band = "-" if cls < 0 else (["apart", "deep"][cls] if cls < 2 else f"band {cls - 2} {'+' if cs['sign'][i] else '-'}")
    return (f"row {i}, class {band}, tilt {cs['tilt'][i]:.3g} (band {int(cs['tilt_band'][i])}), gap {cs['gap'][i]:.3g}, "
            f"kind {int(cs['kind'][i])}, pair {pair.tolist()}")


def check_set(name, out):
    """Items 1-6 of the set on the kernels' answers `out` -> (failures, figures).  Every item is checked whatever
    the others say, so that one run shows them all."""
    cs, m, k = dc.case_set(name), dc.model_of(name), dc.poses(name)
    pairs, ia, ib = out["pairs"], out["ia"], out["ib"]
    N, P = dc.N, len(pairs)
    rows = np.arange(N)
    ex = dc.expected(name, pairs, ia, ib)
    E, col = ex["E"], ex["col"]
    gt = np.asarray(m.geom_type)
    gs = np.asarray(m.geom_size, float).reshape(-1, 3)
    t1, t2 = cs["t1"], cs["t2"]
    bad, fig = [], {}

    def fail(msg):
        bad.append(f"{name}: {msg}")

    # 1. distances
    D = out["D"]
    assert D.shape == (N, P)
    if not np.isfinite(D).all():
        i, p = np.argwhere(~np.isfinite(D))[0]
        fail(f"a distance is not finite at {_where(cs, i, pairs[p])}")
    err = np.where(np.isfinite(D), np.abs(D - E), np.inf)
    i, p = np.unravel_index(np.argmax(err), err.shape)
    fig["dist_err"] = float(err.max())
    fig["dist_err_target"] = float(err[rows, col].max())
    if err.max() > TOL:
        fail(f"|D - E| = {err.max():.3e} (D = {D[i, p]:.12e}, E = {E[i, p]:.12e}, {int((err > TOL).sum())} entries above "
             f"{TOL:g}, target pair: {bool(col[i] == p)}) at {_where(cs, i, pairs[p])}")

    # 2. sign and contact bit against the longdouble verdict
    V = dc.verdicts(name, pairs, ex["Eref"])
    clear_cut = np.abs(E) > TOL
    for what, got in (("D <= 0", D <= 0), ("the contact bit", out["hits"])):
        wrong = clear_cut & (got != V)
        if wrong.any():
            i, p = np.argwhere(wrong)[0]
            fail(f"{what} disagrees with the longdouble verdict on {int(wrong.sum())} entries, first (E = {E[i, p]:.3e}) at "
                 f"{_where(cs, i, pairs[p])}")

    # 3. clearance: bit-identical to the minimum of the distances
    C_, cp = out["clear"]
    want_C, want_pair = ref.clearance_from(D, np.zeros(P), np.zeros(P, bool))
    if C_.tobytes() != want_C.tobytes() or not np.array_equal(cp, want_pair):
        fail("clearance is not the minimum of the distances, lowest index on ties")

    # 4. near pairs: every pair listed, in order, with the distances' bytes
    count, pair, dist, grad, fromto, normal, status = out["near"]
    if not (np.all(count == P) and np.array_equal(pair, np.tile(np.arange(P, dtype=pair.dtype), (N, 1)))):
        fail("near_pairs does not list every pair in ascending order")
    if dist.tobytes() != D.tobytes():
        fail("near_pairs' distances are not mjpl_distances' bytes")
    ok, deg = status == eng_mod.GRAD_OK, status == eng_mod.GRAD_DEGENERATE
    if not np.all(ok | deg):
        fail(f"a status other than OK / DEGENERATE: {np.unique(status).tolist()}")
    # OK slots: witnesses on their geoms, |n| = 1, w2 - w1 = D n, the gradient
    res = np.zeros((N, P))
    for p in range(P):
        r = ok[:, p]
        if not r.any():
            continue
        g1, g2 = pairs[p]
        w1, w2, n = fromto[r, p, :3], fromto[r, p, 3:], normal[r, p]
        for g, w, which in ((g1, w1, 1), (g2, w2, 2)):
            sd = np.abs(gref.point_geom_distance(int(gt[g]), k["geom_xpos"][r, g], k["geom_xmat"][r, g], gs[g], w))
            res[r, p] = np.maximum(res[r, p], sd)
            if sd.max() > WITNESS_TOL:
                i = rows[r][np.argmax(sd)]
                fail(f"witness {which} off its geom by {sd.max():.3e} at {_where(cs, i, pairs[p])}")
        un = np.abs(np.linalg.norm(n, axis=1) - 1)
        if un.max() > UNIT_TOL:
            fail(f"|n| - 1 = {un.max():.3e} at {_where(cs, rows[r][np.argmax(un)], pairs[p])}")
        id_ = np.abs((w2 - w1) - D[r, p, None] * n).max(axis=1)
        res[r, p] = np.maximum(res[r, p], id_)
        if id_.max() > WITNESS_TOL:
            fail(f"|w2 - w1 - D n| = {id_.max():.3e} at {_where(cs, rows[r][np.argmax(id_)], pairs[p])}")
        fk_r = {key: v[r] for key, v in k.items()}
        want = gref.clearance_gradient(m, cs["Q"][r], np.tile(pairs[p], (int(r.sum()), 1)), fromto[r, p], n, fk=fk_r)
        ge = np.abs(grad[r, p] - want).max(axis=1)
        fig["grad_err"] = max(fig.get("grad_err", 0.0), float(ge.max()))
        if not ge.max() <= WITNESS_TOL:
            fail(f"|grad - n . (J2 - J1)| = {ge.max():.3e} at {_where(cs, rows[r][np.argmax(ge)], pairs[p])}")
    fig["witness_res"] = float(res.max())
    # DEGENERATE slots: no direction, the two core points
    if deg.any():
        if not (np.isnan(grad[deg]).all() and np.isnan(normal[deg]).all() and np.isfinite(fromto[deg]).all()):
            fail("a DEGENERATE slot with a gradient or a normal, or without its points")
        sep = np.abs(fromto[deg][:, 3:] - fromto[deg][:, :3]).max()
        if not sep <= WITNESS_TOL:
            fail(f"a DEGENERATE slot whose points are {sep:.3e} apart")
    # status by core gap (the decade around the header's 1e-10 is free)
    core = ex["coregap"]
    wrong = (core > 1e-9) & ~ok
    if wrong.any():
        i, p = np.argwhere(wrong)[0]
        fail(f"{int(wrong.sum())} slots with a core gap above 1e-9 are not OK, first (core gap {core[i, p]:.3e}) at "
             f"{_where(cs, i, pairs[p])}")
    wrong = deg & ~(core < 1e-9)
    if wrong.any():
        i, p = np.argwhere(wrong)[0]
        fail(f"{int(wrong.sum())} DEGENERATE slots have a core gap of 1e-9 or more, first ({core[i, p]:.3e}) at "
             f"{_where(cs, i, pairs[p])}")
    # family C: the statuses and depths the construction fixes
    want_st = cs["want_status"]
    has = want_st >= 0
    if has.any() and not np.array_equal(status[rows, col][has], want_st[has]):
        i = rows[has][np.argmax(status[rows, col][has] != want_st[has])]
        fail(f"target status {int(status[i, col[i]])}, want {int(want_st[i])}, at {_where(cs, i, pairs[col[i]])}")
    closed = np.isfinite(cs["closed"])
    if closed.any():
        ce = np.abs(D[rows, col] - cs["closed"])[closed]
        if not ce.max() <= CLOSED_TOL:
            i = rows[closed][np.argmax(ce)]
            fail(f"|D - closed form| = {ce.max():.3e} at {_where(cs, i, pairs[col[i]])}")

    # 5. clearance_grad: the near-pairs slot of the pair it picked, bit for bit, in all six outputs
    gC, gp, gg, gf, gn, gst = out["cgrad"]
    if gC.tobytes() != C_.tobytes() or not np.array_equal(gp, cp):
        fail("clearance_grad's clearance or pair differ from mjpl_clearance's")
    else:
        for what, a, b in (("grad", gg, grad[rows, gp]), ("fromto", gf, fromto[rows, gp]), ("normal", gn, normal[rows, gp]),
                           ("status", gst, status[rows, gp])):
            if a.tobytes() != np.ascontiguousarray(b).tobytes():
                fail(f"clearance_grad's {what} differs from the near-pairs slot of its pair")

    # 6. overlapping target pairs: D is the length of a separating translation along n
    tgt_ok = ok[rows, col] & V[rows, col] & np.isfinite(normal[rows, col]).all(axis=1)
    if tgt_ok.any():
        r = rows[tgt_ok]
        g1, g2 = pairs[col[r], 0], pairs[col[r], 1]
        p1, R1 = dc._ld_pose({key: v[r] for key, v in k.items()}, g1)
        p2, R2 = dc._ld_pose({key: v[r] for key, v in k.items()}, g2)
        s1, s2 = gs[g1].astype(LD), gs[g2].astype(LD)
        n, depth = normal[r, col[r]].astype(LD), np.abs(D[r, col[r]]).astype(LD)
        for step, want_touch in ((STEP, False), (-STEP, True)):
            moved = p2 + (depth + LD(step))[:, None] * n
            touch = np.asarray(nc.gap(t1, p1, R1, s1, t2, moved, R2, s2) <= 0)
            if not np.all(touch == want_touch):
                i = r[np.argmax(touch != want_touch)]
                what = "still overlaps" if step > 0 else "no longer overlaps"
                fail(f"geom 2 moved by |D| {'+' if step > 0 else '-'} {STEP:g} along n {what} on "
                     f"{int((touch != want_touch).sum())} of {len(r)} rows, first (D = {D[i, col[i]]:.6e}) at "
                     f"{_where(cs, i, pairs[col[i]])}")
    fig["overlapping_targets"] = int(tgt_ok.sum())
    return bad, fig


@pytest.mark.parametrize("name", dc.SETS)
def test_set(name):
    out = run_engine(name)
    bad, fig = check_set(name, out)
    print(f"MEASURED {name}: |D - E| {fig['dist_err']:.3e} (target pairs {fig['dist_err_target']:.3e}), witness "
          f"residual {fig['witness_res']:.3e}, gradient {fig.get('grad_err', 0.0):.3e}, overlapping targets "
          f"{fig['overlapping_targets']}")
    assert not bad, "\n".join(bad)


def test_push_out_beside_a_box_edge():
    """push_out shares the routines: 64 rows of the capsule || box edge set, d_min above every gap"""
    name = "A capsule || box edge"
    cs, m = dc.case_set(name), dc.model_of(name)
    Q = np.ascontiguousarray(cs["Q"][:64])
    d_min = 0.15
    assert cs["gap"][:64].max() < d_min
    e = eng_mod.Engine(m)
    assert e.clearance(Q)[0].max() < d_min
    Qo, clear, pair, iters, st = e.push_out(Q, d_min)
    for a in (Qo, clear):
        assert np.isfinite(a).all()
    assert np.all(st != eng_mod.PUSH_NONFINITE)
    assert np.array_equal(st == eng_mod.PUSH_OK, clear >= d_min)
    assert np.all((clear >= d_min - 1e-9) | np.isin(st, PUSH_STATUS_UNMOVED)), (clear.min(), np.bincount(st))
    C_, cp = e.clearance(Qo, d_min)
    assert clear.tobytes() == C_.tobytes() and pair.tobytes() == cp.tobytes()
    print(f"push_out: {int((st == eng_mod.PUSH_OK).sum())} of 64 rows reach {d_min}, statuses {np.bincount(st).tolist()}")
    e.close()
