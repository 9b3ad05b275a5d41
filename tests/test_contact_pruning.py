"""The model compiler's second proving stage: enabled pairs of a moving geom with a static geom or a plane
proved never to come within their contact margin are a side set of the compiled program -- ip / fp / dp, the masks and the
`dropped` list do not know them; a per-program library's generated check leaves them out.  Host only: the set comes from
mjpl_program_dump_never_touch, the poses from the oracle's FK, the verdicts from the oracle's narrowphase.

Soundness is checked by sampling -- which may refute a member of the set, never justify one: the models and the sample of
tests/test_pair_pruning.py (20 000 configurations with every hinge uniform over the full circle, 2 000 more with angles up
to +-6.5 rad, slides uniform over their ranges), no member in contact at its margin plus 1 mm."""
import re

import numpy as np
import pytest

from mjpl_amd import specialise
from mjpl_amd.model import ModelBuilder
from oracle import pyoracle

from test_pair_pruning import MODELS, IDS, _sample

_cache = {}


def _never(k, **kw):
    name, model, allowed, qidx, base = MODELS[k]
    return specialise.dump_never_touch(model, allowed, qidx, base, **kw)


def _case(k):
    """(never-touch pairs of model k as a set of tuples, the raw result) -- computed once."""
    if k not in _cache:
        res = _never(k)
        _cache[k] = ({(int(a), int(b)) for a, b in res[0]}, res)
    return _cache[k]


def _names(model, pairs):
    return {frozenset((model.geom_names[a], model.geom_names[b])) for a, b in pairs}


def _in_contact(model, fk, g1, g2, extra):
    """Configurations of the sample where the oracle's narrowphase reports the pair in contact at its margin + extra."""
    margin = max(model.geom_margin[g1], model.geom_margin[g2]) + extra
    t1, t2, s1, s2 = int(model.geom_type[g1]), int(model.geom_type[g2]), model.geom_size[g1], model.geom_size[g2]
    X, M = fk["geom_xpos"], fk["geom_xmat"]
    return [n for n in range(len(X)) if pyoracle.pair_test(t1, X[n, g1], M[n, g1], s1, t2, X[n, g2], M[n, g2], s2, margin) != 0]


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_no_pair_of_the_set_is_in_contact_in_the_sample(k):
    name, model, allowed, qidx, base = MODELS[k]
    pairs, _ = _case(k)
    if not pairs:
        return
    fk = pyoracle.Oracle(model, allowed).fk(_sample(model, 100 + k))
    for g1, g2 in sorted(pairs):
        assert g1 < g2
        hits = _in_contact(model, fk, g1, g2, 1e-3)
        assert not hits, (name, model.geom_names[g1], model.geom_names[g2], len(hits))


def test_benchmark_model_contents():
    model = MODELS[0][1]
    pairs, (_, evals, h, th) = _case(0)
    names = _names(model, pairs)
    assert frozenset(("link0_c", "link1_c")) in names and frozenset(("obstacle_3", "link3_c")) in names, names
    assert 0 < evals <= 1 << 18 and h != th


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_only_pairs_with_a_static_geom_and_none_of_the_dropped_list(k):
    name, model, allowed, qidx, base = MODELS[k]
    pairs, _ = _case(k)
    static = model.body_weldid[model.geom_bodyid] == 0
    for g1, g2 in pairs:
        assert static[g1] != static[g2], (name, g1, g2)
    for level in (1, 2):
        dropped = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=level)[4]
        assert not pairs & {tuple(p) for p in dropped.tolist()}, name
    # (the self pairs stage 1b drops at level 2 do not change what this stage finds)
    assert {tuple(p) for p in _never(k, prune_pairs=2)[0].tolist()} == pairs


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_planning_selection_does_not_change_the_set(k):
    name, model, allowed, qidx, base = MODELS[k]
    want = _case(k)[1][0]
    rng = np.random.default_rng(7 + k)
    lo, hi = model.jnt_range[:, 0], model.jnt_range[:, 1]
    other_base = np.where(hi > lo, rng.uniform(lo, hi), np.asarray(base, float))
    selections = [(np.arange(model.nq, dtype=np.int32), other_base), (np.arange(model.nq, dtype=np.int32)[::-1][:max(1, model.nq // 2)].copy(), other_base),
                  (np.asarray(qidx, np.int32)[:1], np.asarray(base, float))]
    for sel, b in selections:
        np.testing.assert_array_equal(specialise.dump_never_touch(model, allowed, sel, b)[0], want, err_msg=name)


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_tables_untouched_and_hash_differs_exactly_when_the_set_is_not_empty(k):
    """ip / fp / dp with the option on and off: one hash of the three tables (which covers every byte of them), and the
    tables dump_program_pruned returns are the same call's; the program hash moves exactly when the set is not empty."""
    name, model, allowed, qidx, base = MODELS[k]
    pairs, (_, _, h_on, tables_on) = _case(k)
    off_pairs, off_evals, h_off, tables_off = _never(k, prune_contacts=0)
    assert len(off_pairs) == 0 and off_evals == 0
    assert tables_on == tables_off == h_off
    assert (h_on != h_off) == bool(pairs), name
    info = specialise.dump_program_pruned(model, allowed, qidx, base, prune_pairs=1)[3]
    assert int(info.hash) == h_on == int(specialise.dump_program(model, allowed, qidx, base)[3].hash)


def _stage_geoms(ip):
    out, pc = [], int(ip[specialise.H_OFF_BODYOPS])
    for _ in range(int(ip[specialise.H_NBODYOPS])):
        njnt, ngeom = int(ip[pc + specialise.B_NJNT]), int(ip[pc + specialise.B_NGEOM])
        pc += specialise.B_SIZE + njnt * specialise.J_SIZE
        for _ in range(ngeom):
            out.append(int(ip[pc + specialise.G_GEOMID]))
            pc += specialise.G_SIZE + specialise.MAX_SLOTS
    return out


@pytest.mark.parametrize("k", range(len(MODELS)), ids=IDS)
def test_generated_source_leaves_exactly_the_set_out(k):
    name, model, allowed, qidx, base = MODELS[k]
    pairs, _ = _case(k)
    ip, fp, dp, info = specialise.dump_program(model, allowed, qidx, base)
    full = specialise.generate(ip, fp, dp, info)
    src = specialise.generate(ip, fp, dp, info, never_touch=sorted(pairs))

    def literal(s):
        return int(re.search(r"(\d+) literal pairs", s).group(1))
    assert literal(full) - literal(src) == len(pairs), name
    # no descriptor of a static or plane partner names a member of the set (world rows: static geoms in geom-id order)
    static = model.body_weldid[model.geom_bodyid] == 0
    row_geom = [int(g) for g in np.flatnonzero(static)]
    words = [int(x) for x in re.search(r"kSpecDesc\[[^\]]*\] = \{(.*?)\};", src, re.S).group(1).replace("\n", " ").split(",") if x.strip()]
    geoms = _stage_geoms(ip)
    assert len(words) == 64 * len(geoms)
    seen = 0
    for si, g in enumerate(geoms):
        for x in words[64 * si: 64 * si + 64]:
            if x and (x & 3) in (specialise.EK_PLANE, specialise.EK_STATIC):
                partner = row_geom[(x >> 2) & 255]
                assert (min(g, partner), max(g, partner)) not in pairs, (name, g, partner)
                seen += 1
    assert seen > 0
    # ... and a scene-generic library is generated as before
    if info.scene_ok:
        assert specialise.generate(ip, fp, dp, info, generic=True, never_touch=sorted(pairs)) == specialise.generate(ip, fp, dp, info, generic=True)


# ---- two-body models: one hinge about z at the origin, a capsule along the link's x axis (core from x = 0.05 to 0.35,
# radius 0.03) swinging in the plane z = 0 past a static geom on the x axis.  The cores come closest at angle 0.
_REACH, _R = 0.35, 0.03


def _swing(partner: str, clearance: float):
    mb = ModelBuilder()
    mb.add_body("arm", "world")
    mb.add_joint("arm", "hinge", "hinge", axis=(0, 0, 1), range=(-3.0, 3.0))
    mb.add_geom("arm", "capsule", (_R, 0.15), pos=(0.2, 0, 0), quat=(np.sqrt(0.5), 0, np.sqrt(0.5), 0), name="swing")
    if partner == "upright capsule":      # core: the segment x = X, y = 0, |z| <= 0.2
        mb.add_geom("world", "capsule", (0.04, 0.2), pos=(_REACH + _R + 0.04 + clearance, 0, 0), name="post")
    elif partner == "skew capsule":       # core: a segment through (X, 0, 0) in the plane x = X, tilted about x
        mb.add_geom("world", "capsule", (0.04, 0.2), pos=(_REACH + _R + 0.04 + clearance, 0, 0),
                    quat=(np.cos(0.4), np.sin(0.4), 0, 0), name="post")
    else:                                 # a box whose face x = X - 0.05 faces the hinge
        mb.add_geom("world", "box", (0.05, 0.06, 0.07), pos=(_REACH + _R + 0.05 + clearance, 0, 0), name="post")
    return mb.compile()


@pytest.mark.parametrize("partner", ["upright capsule", "skew capsule", "box"])
def test_two_body_models(partner):
    def never(clearance):
        m = _swing(partner, clearance)
        pairs = specialise.dump_never_touch(m)[0]
        # (the pair passes its bounding cull -- else stage 1b owns it and this stage never sees it)
        assert len(specialise.dump_program_pruned(m, prune_pairs=1)[4]) == 0
        return _names(m, pairs)
    assert never(0.02) == {frozenset(("swing", "post"))}          # 2 cm of clearance: proved
    assert never(-0.005) == set()                                 # touches around angle 0: kept
    assert never(0.0005) == set()                                 # clear by half a millimetre: under the slack, kept
    m = _swing(partner, -0.005)
    q = np.array([[0.0], [np.pi]])
    assert list(pyoracle.Oracle(m).valid_configs(q)) == [False, True]  # (the touching twin does touch, and only near 0)


def _planar_chain(nlinks: int):
    """nlinks - 1 hinges about z and a last one about the link's own x axis, 2 cm apart; the last link's capsule lies along
    x, in the plane z = 0, 10 cm below a small static sphere whatever the angles -- and within its bounding radius of it
    when the chain folds back over the origin."""
    mb = ModelBuilder()
    mb.add_geom("world", "sphere", (0.03,), pos=(0, 0, 0.15), name="ball")
    for b in range(nlinks):
        mb.add_body(f"l{b}", f"l{b - 1}" if b else "world", pos=(0.02 if b else 0.0, 0, 0))
        mb.add_joint(f"l{b}", f"j{b}", "hinge", axis=(0, 0, 1) if b < nlinks - 1 else (1, 0, 0), range=(-3.0, 3.0))
    mb.add_geom(f"l{nlinks - 1}", "capsule", (0.02, 0.12), pos=(0.02, 0, 0), quat=(np.sqrt(0.5), 0, np.sqrt(0.5), 0), name="tip")
    return mb.compile()


def test_hinge_limit_and_budget():
    for nlinks, want in ((3, {frozenset(("ball", "tip"))}), (4, set())):  # (the stage covers three hinges)
        m = _planar_chain(nlinks)
        assert len(specialise.dump_program_pruned(m, prune_pairs=1)[4]) == 0
        assert _names(m, specialise.dump_never_touch(m)[0]) == want, nlinks
    # a pair whose proof needs more cell evaluations than it may spend is kept: the benchmark model with 64 per pair
    model = MODELS[0][1]
    pairs, (_, evals, _, _) = _case(0)
    small, small_evals, _, _ = _never(0, prune_contacts=64)
    small = {(int(a), int(b)) for a, b in small}
    assert small < pairs and frozenset(("obstacle_3", "link3_c")) not in _names(model, small)
    assert 0 < small_evals < evals


def test_plane_partner():
    """The same swinging capsule 2 cm above a floor (kept when it dips 5 mm into it), beside a post it does touch: the plane
    pair is proved, the generated source loses exactly that pair and keeps no plane descriptor."""
    def model(clearance):
        mb = ModelBuilder()
        mb.add_geom("world", "plane", (1, 1, 0.1), pos=(0, 0, -_R - clearance), name="floor")
        mb.add_geom("world", "capsule", (0.04, 0.2), pos=(_REACH + _R + 0.04 - 0.005, 0, 0), name="post")
        mb.add_body("arm", "world")
        mb.add_joint("arm", "hinge", "hinge", axis=(0, 0, 1), range=(-3.0, 3.0))
        mb.add_geom("arm", "capsule", (_R, 0.15), pos=(0.2, 0, 0), quat=(np.sqrt(0.5), 0, np.sqrt(0.5), 0), name="swing")
        return mb.compile()
    m = model(0.02)
    assert len(specialise.dump_program_pruned(m, prune_pairs=1)[4]) == 0
    pairs = specialise.dump_never_touch(m)[0]
    assert _names(m, pairs) == {frozenset(("floor", "swing"))}
    assert _names(model(-0.005), specialise.dump_never_touch(model(-0.005))[0]) == set()
    ip, fp, dp, info = specialise.dump_program(m)
    full, src = specialise.generate(ip, fp, dp, info), specialise.generate(ip, fp, dp, info, never_touch=pairs)

    def words(s):
        return [int(x) for x in re.search(r"kSpecDesc\[[^\]]*\] = \{(.*?)\};", s, re.S).group(1).replace("\n", " ").split(",") if x.strip()]
    plane = [x for x in words(full) if x and (x & 3) == specialise.EK_PLANE]
    assert len(plane) == 1 and not [x for x in words(src) if x and (x & 3) == specialise.EK_PLANE]
    assert sum(1 for x in words(full) if x) - sum(1 for x in words(src) if x) == 1
    assert full.count("MJPL_SPEC_HIT(") - src.count("MJPL_SPEC_HIT(") == 1
