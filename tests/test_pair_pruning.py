"""The model compiler's pruning stage: enabled pairs proved never to pass their bounding cull are left
out of the compiled program.  Host only: the program comes from mjpl_program_dump_pruned, the poses from the oracle's FK.

Soundness is checked by sampling -- which may refute a drop, never justify one: every dropped pair stays outside its
bounding radii and margin at 20 000 configurations with every hinge uniform over the full circle and 2 000 more with
angles up to +-6.5 rad (what the check accepts as |dq|), slides uniform over their ranges."""
import hashlib
import json
import os

import numpy as np
import pytest

from mjpl_amd import scenes, specialise
from mjpl_amd.model import GEOM_PLANE, JNT_SLIDE
from oracle import pyoracle

from spec_models import spec_models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "program_digests.json")
N_CIRCLE, N_WIDE = 20000, 2000


def _models():
    """The benchmark model, UR5e and the random models of tests/spec_models.py: (name, model, allowed, qidx, base)."""
    keep = [e for e in spec_models() if e[0].startswith(("franka_p+16obs, arm planned", "ur5e", "random_model"))]
    assert len(keep) == 6
    return keep


MODELS = _models()
IDS = [e[0].split(",")[0].split(" (")[0] for e in MODELS]


def _sample(model, seed):
    rng = np.random.default_rng(seed)
    nq = model.nq
    Q = np.concatenate([rng.uniform(-np.pi, np.pi, size=(N_CIRCLE, nq)), rng.uniform(-6.5, 6.5, size=(N_WIDE, nq))])
    for j in range(model.njnt):
        if model.jnt_type[j] == JNT_SLIDE:
            a = model.jnt_qposadr[j]
            lo, hi = model.jnt_range[j]
            if not hi > lo:
                lo, hi = -1.0, 1.0
            Q[:, a] = rng.uniform(lo, hi, size=len(Q))
    return Q


_cache = {}


def _case(k):
    """Dropped pairs of model k -- at level 2 of the option, self pairs included: a superset of the default's -- and the
    oracle's geom poses at the sample: computed once, shared, never written to."""
    if k not in _cache:
        name, model, allowed, qidx, base = MODELS[k]
        dropped = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=2)[4]
        fk = pyoracle.Oracle(model, allowed).fk(_sample(model, 100 + k))
        fk["geom_xpos"].setflags(write=False)
        fk["geom_xmat"].setflags(write=False)
        _cache[k] = (dropped, fk)
    return _cache[k]


def _gaps(model, fk, g1, g2):
    """distance - radii - margin of the pair's bounding cull at every sampled configuration (a plane: signed height)."""
    margin = max(model.geom_margin[g1], model.geom_margin[g2])
    x1, x2 = fk["geom_xpos"][:, g1], fk["geom_xpos"][:, g2]
    if model.geom_type[g1] == GEOM_PLANE or model.geom_type[g2] == GEOM_PLANE:
        p, o = (g1, g2) if model.geom_type[g1] == GEOM_PLANE else (g2, g1)
        normal = fk["geom_xmat"][:, p].reshape(-1, 3, 3)[:, :, 2]
        return np.einsum("nk,nk->n", normal, fk["geom_xpos"][:, o] - fk["geom_xpos"][:, p]) - model.geom_rbound[o] - margin
    return np.linalg.norm(x1 - x2, axis=1) - model.geom_rbound[g1] - model.geom_rbound[g2] - margin


def _joints_between(model, g1, g2):
    """The joints the pair's relative pose depends on: those of the bodies on exactly one of the two root paths."""
    def path(g):
        out, b = set(), int(model.geom_bodyid[g])
        while b > 0:
            out.add(b)
            b = int(model.body_parentid[b])
        return out
    joints = []
    for b in path(g1) ^ path(g2):
        joints += range(int(model.body_jntadr[b]), int(model.body_jntadr[b]) + int(model.body_jntnum[b]))
    return joints


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_dropped_pairs_never_pass_their_cull(k):
    model = MODELS[k][1]
    dropped, fk = _case(k)
    for g1, g2 in dropped:
        assert g1 < g2
        gap = _gaps(model, fk, int(g1), int(g2))
        assert gap.min() > 0, (MODELS[k][0], model.geom_names[g1], model.geom_names[g2], float(gap.min()))
        assert all(model.jnt_type[j] != JNT_SLIDE for j in _joints_between(model, int(g1), int(g2)))


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_planning_selection_does_not_change_the_decisions(k):
    name, model, allowed, qidx, base = MODELS[k]
    want = _case(k)[0]
    rng = np.random.default_rng(7 + k)
    lo, hi = model.jnt_range[:, 0], model.jnt_range[:, 1]
    other_base = np.where(hi > lo, rng.uniform(lo, hi), np.asarray(base, float))
    selections = [(np.arange(model.nq, dtype=np.int32), other_base), (np.arange(model.nq, dtype=np.int32)[::-1][:max(1, model.nq // 2)].copy(), other_base),
                  (np.asarray(qidx, np.int32)[:1], np.asarray(base, float))]
    for sel, b in selections:
        got = specialise.dump_program_pruned(model, allowed, sel, b, prune_pairs=2)[4]
        np.testing.assert_array_equal(got, want, err_msg=name)


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_default_level_drops_pairs_with_static_geoms_only(k):
    name, model, allowed, qidx, base = MODELS[k]
    both = {tuple(p) for p in _case(k)[0].tolist()}
    static = model.body_weldid[model.geom_bodyid] == 0
    level1 = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=1)[4]
    assert {tuple(p) for p in level1.tolist()} == {p for p in both if static[p[0]] != static[p[1]]}, name


def test_benchmark_model_drops_the_unreachable_obstacle_pairs():
    name, model, allowed, qidx, base = MODELS[0]
    fk = _case(0)[1]
    dropped = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=1)[4]
    is_obstacle = np.array([n.startswith("obstacle_") for n in model.geom_names])
    assert int(is_obstacle.sum()) == 16
    obstacle = [(a, b) for a, b in dropped if is_obstacle[a] != is_obstacle[b]]
    # 53 fall to the fixed anchor of their chain alone, 6 more to the bisection over at most three proximal hinges
    assert len(obstacle) >= 59, len(obstacle)
    # the two most proximal moving links are out of reach of all 16 obstacles
    for link in ("link1_c", "link2_c"):
        g = model.geom(link).id
        assert sum(1 for a, b in obstacle if g in (a, b)) == 16, link
    # ... and nothing is dropped that the sample shows within its radii (the enabled pairs that do pass stay in the program)
    ip1 = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=1)[0]
    ip0 = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=0)[0]
    assert ip1.shape == ip0.shape and (ip1 != ip0).any()
    for g1, g2 in dropped:
        assert _gaps(model, fk, int(g1), int(g2)).min() > 0
    # level 2 adds self pairs of the arm (only the joints between the two geoms count)
    assert len(_case(0)[0]) > len(dropped)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_switch_off_gives_the_program_of_an_empty_drop_list():
    """prune_pairs = 0: ip / fp / dp are those of a compile that drops nothing -- the digests recorded from the compiler
    before it had the stage (tests/golden/program_digests.json; a change of the table layout or of a constant of these
    models changes them: tools/make_program_digests.py writes the file again, from the compile that drops nothing) -- and where the stage proves nothing, on equals off."""
    golden = json.load(open(GOLDEN))
    seen_empty = False
    for name, model, allowed, qidx, base in MODELS + [e for e in spec_models() if e[0].startswith("two_dof_ball")]:
        ip0, fp0, dp0, info0, dropped0 = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=0)
        assert len(dropped0) == 0
        key = name.split(" (")[0]
        assert {"ip": _digest(ip0), "fp": _digest(fp0), "dp": _digest(dp0)} == golden[key], name
        ip1, fp1, dp1, info1, dropped1 = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=1)
        dflt = specialise.dump_program(model, allowed, qidx, base)
        assert int(dflt[3].hash) == int(info1.hash), "the default program is the pruned one"
        if len(dropped1) == 0:
            seen_empty = True
            assert int(info1.hash) == int(info0.hash)
            for a, b in ((ip0, ip1), (fp0, fp1), (dp0, dp1)):
                np.testing.assert_array_equal(a, b)
        else:
            assert int(info1.hash) != int(info0.hash)
    assert seen_empty


def test_dropped_pairs_stay_in_the_pair_counts_and_leave_the_masks():
    """The per-geom masks of the program lose exactly the dropped static partners; sizes and offsets of the tables stay."""
    name, model, allowed, qidx, base = MODELS[0]
    ip1, _, dp1, _, dropped = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=1)
    ip0, _, dp0, _, _ = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=0)
    assert len(dp1) == len(dp0)

    def masks(ip):
        out, pc = {}, int(ip[specialise.H_OFF_BODYOPS])
        for _ in range(int(ip[specialise.H_NBODYOPS])):
            njnt, ngeom = int(ip[pc + specialise.B_NJNT]), int(ip[pc + specialise.B_NGEOM])
            pc += specialise.B_SIZE + njnt * specialise.J_SIZE
            for _ in range(ngeom):
                w = [int(ip[pc + f]) & 0xFFFFFFFF for f in (specialise.G_WMASK_LO, specialise.G_WMASK_HI, specialise.G_PMASK_LO, specialise.G_PMASK_HI)]
                out[int(ip[pc + specialise.G_GEOMID])] = (w[0] | w[1] << 32) | (w[2] | w[3] << 32)
                pc += specialise.G_SIZE + specialise.MAX_SLOTS
        return out
    m1, m0 = masks(ip1), masks(ip0)
    static = model.body_weldid[model.geom_bodyid] == 0
    rows = {int(g): r for r, g in enumerate(np.flatnonzero(static))}  # world rows in geom-id order
    for g in m0:
        gone = sum(1 << rows[int(a if static[a] else b)] for a, b in dropped if g in (a, b) and static[a] != static[b])
        assert m1[g] == m0[g] & ~gone and m0[g] & gone == gone, model.geom_names[g]
