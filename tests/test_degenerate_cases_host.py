"""The touching, aligned and coincident pose families of tests/degenerate_cases.py, the parts that need no GPU: the
recipe's digest per set, that every class, band and sign is populated, that the oracle's forward kinematics
reproduces the requested poses through the pods of tests/pose_pods.py, that aligned rows carry bit-identical
matrices, that the model compiler keeps every pair, and that the two reference statements -- the NumPy one of
tests/distance_reference.py and the longdouble one of tests/narrowphase_cases.py -- agree where both apply.
tests/test_gpu_degenerate_poses.py runs the same sets through the kernels."""
import numpy as np
import pytest

import degenerate_cases as dc
import narrowphase_cases as nc
import pose_pods as pods
from mjpl_amd import specialise

# sha256 of Q (first 16 hex digits) per set: a change of recipe shows here
DIGESTS = {
    "T plane-sphere": "4236cdc2b3d48b58",
    "T plane-capsule": "f86bc498d0034150",
    "T plane-box": "c7319021ac5c3fd7",
    "T sphere-sphere": "90fe37751f5a43c7",
    "T sphere-capsule": "f0ac615ac50ba61a",
    "T capsule-capsule": "00ab7a12236cdf05",
    "T sphere-box": "856c08b0dbae7119",
    "T capsule-box": "414650815a8ae0cc",
    "T box-box": "0ab29e90011f43a2",
    "A capsule || capsule": "281ed90ef5a413db",
    "A capsule || box edge": "d9a3e1fec87621d8",
    "A capsule || box face": "d28bcf364c21f6f8",
    "A box || box": "9949895b94ad1239",
    "A plane || box face": "1bfc197206b22486",
    "A plane || capsule axis": "2e2450b5843c7cb5",
    "A sphere on box Voronoi boundaries": "b758a0d159f852f6",
    "C concentric spheres": "43330a6753f8ba8f",
    "C sphere centre on capsule axis": "8f156fe804de3a88",
    "C capsule axes crossing": "b80467221d208047",
    "C sphere centre on box face": "cb78f0a28f6c73fb",
    "C capsule through box centre": "9e44490e7c49908c",
    "C boxes with a common centre": "af61985801482747",
}
N = dc.N
SHARE = 0.85     # of the target pairs of a T or A set, the part that gets the longdouble comparison
AGREE = 1e-12    # |NumPy statement - longdouble statement| where both apply


def test_the_sets():
    assert list(DIGESTS) == dc.SETS
    assert sum(s.startswith("T ") for s in dc.SETS) == len(nc.PAIRS) == 9


def test_a_pod_frame_is_rx_ry_rz_of_its_hinges():
    rng = np.random.default_rng(3)
    R = nc.quat_mat64(rng.normal(size=(256, 4)))
    ang = pods.euler_xyz(R)
    assert np.abs(pods.rot_xyz(ang) - R).max() <= 1e-14
    m = pods.two_pod_model(dc.SPHERE, [[0.1, 0, 0]], dc.BOX, [[0.1, 0.2, 0.3]])
    p = rng.uniform(-1, 1, (256, 3))
    k = pods.fk(m, pods.configs(p, R, -p, R[::-1]))
    ga, gb = pods.pod_geoms(m)
    assert np.array_equal(k["geom_xpos"][:, ga[0]], p) and np.array_equal(k["geom_xpos"][:, gb[0]], -p)
    assert np.abs(k["geom_xmat"][:, ga[0]].reshape(-1, 3, 3) - pods.rot_xyz(ang)).max() <= 1e-14
    assert np.abs(k["geom_xmat"][:, gb[0]].reshape(-1, 3, 3) - R[::-1]).max() <= 1e-13


@pytest.mark.parametrize("name", dc.SETS)
def test_digest_and_population(name):
    cs = dc.case_set(name)
    assert cs["Q"].shape == (N, 6 if cs["t1"] == dc.PLANE else 12) and np.isfinite(cs["Q"]).all()
    assert dc.digest(cs) == DIGESTS[name], "the recipe changed: bump degenerate_cases.RECIPE and the digests"
    for who, g in (("tgt_a", 1 if cs["t1"] == dc.PLANE else dc.G), ("tgt_b", dc.G)):
        for k in range(g):
            assert (cs[who] == k).sum() > N // (4 * g)  # every pair of the row is the target somewhere
    if cs["family"] == "T":
        for k in range(8):
            assert (cs["cls"] == k).sum() > N // 16, (name, k)
        band = cs["cls"] >= nc.BAND0
        assert (band & cs["sign"]).sum() > N // 16 and (band & ~cs["sign"]).sum() > N // 16
    if cs["family"] == "A":
        for k in range(7):
            assert (cs["tilt_band"] == k).sum() > N // 16, (name, k)
        assert np.all((cs["tilt"] == 0) == (cs["tilt_band"] == 0))
        for k in range(4):  # the gap's decades, in pairs
            assert ((cs["gap"] >= 10.0 ** (2 * k - 9)) & (cs["gap"] < 10.0 ** (2 * k - 7))).sum() > N // 16, (name, k)
    for k in np.unique(cs["kind"]):
        assert (cs["kind"] == k).sum() > N // 16, (name, k)


@pytest.mark.parametrize("name", dc.SETS)
def test_oracle_fk_reproduces_the_requested_poses(name):
    cs, m, k = dc.case_set(name), dc.model_of(name), dc.poses(name)
    ga, gb = pods.pod_geoms(m)
    assert len(gb) == dc.G and len(ga) == (1 if cs["t1"] == dc.PLANE else dc.G)
    assert m.nq == cs["Q"].shape[1]
    for who, ids in (("1", ga), ("2", gb)):
        for g in ids:
            assert np.abs(k["geom_xpos"][:, g] - cs["p" + who]).max() <= 1e-12, (name, who)
            assert np.abs(k["geom_xmat"][:, g].reshape(N, 3, 3) - cs["R" + who]).max() <= 1e-12, (name, who)
    # the geoms of one pod share its pose bit for bit; a pod's centre is its slide values themselves
    assert np.array_equal(k["geom_xmat"][:, gb[0]], k["geom_xmat"][:, gb[1]])
    assert np.array_equal(k["geom_xpos"][:, gb[0]], cs["Q"][:, -6:-3])
    # aligned rows: the same hinge values in both pods, so the same arithmetic and the same bits
    al = cs["aligned"]
    if al.any():
        assert np.array_equal(cs["Q"][al, 3:6], cs["Q"][al, 9:12])
        assert np.array_equal(k["geom_xmat"][al][:, ga[0]], k["geom_xmat"][al][:, gb[0]]), name
    if cs["family"] == "A" and cs["t1"] != dc.PLANE and cs["t1"] != dc.SPHERE:
        assert al.sum() > N // 64, name
    if name in ("C concentric spheres", "C boxes with a common centre"):
        assert np.array_equal(k["geom_xpos"][:, ga[0]], k["geom_xpos"][:, gb[0]])


@pytest.mark.parametrize("name", dc.SETS)
def test_the_model_compiler_keeps_every_pair(name):
    m = dc.model_of(name)
    dropped = specialise.dump_program_pruned(m, (), None, None, prune_pairs=2)[4]
    assert len(dropped) == 0, (name, dropped.tolist())
    pairs, ia, ib = dc.host_pairs(name)
    assert {(int(min(p)), int(max(p))) for p in pairs} == pods.product_pairs(m)
    gt = np.asarray(m.geom_type)
    assert np.all(gt[pairs[:, 0]] == dc.case_set(name)["t1"]) and np.all(gt[pairs[:, 1]] == dc.case_set(name)["t2"])


@pytest.mark.parametrize("name", dc.SETS)
def test_the_two_statements_agree(name):
    """|distance_reference - longdouble| <= 1e-12 on every target pair whose cores are apart, the same sign
    everywhere, and enough of the target pairs get the longdouble comparison."""
    cs = dc.case_set(name)
    pairs, ia, ib = dc.host_pairs(name)
    ex = dc.expected(name, pairs, ia, ib)
    rows = np.arange(N)
    use, col = ex["use"], ex["col"]
    ref_t = ex["Eref"][rows, col]
    err = np.abs(ref_t[use] - ex["gap"][use].astype(np.float64))
    worst = float(err.max()) if use.any() else 0.0
    print(f"{name}: longdouble on {use.mean():.3f} of the target pairs, |NumPy - longdouble| = {worst:.2e}")
    assert worst <= AGREE, (name, worst, int(rows[use][np.argmax(err)]))
    clear_cut = np.abs(ref_t) > AGREE
    assert np.array_equal((ref_t <= 0)[clear_cut], np.asarray(ex["gap"] <= 0)[clear_cut]), name
    assert np.isfinite(ex["E"]).all()
    if cs["family"] == "T":
        # the verdict the bisection aimed at (a band pose clipped at s = 0 aside, as narrowphase_cases.solve says)
        want = np.where(cs["cls"] == nc.APART, False, np.where(cs["cls"] == nc.DEEP, True, ~cs["sign"]))
        got = np.asarray(ex["gap"] <= 0)
        assert np.all((got == want) | (cs["s"] == 0.0)), name
    if name == "T box-box":
        # Boxes have no radius: a touching pose has its cores touching, the delta classes put half of the rows on
        # the overlapping side, and no longdouble depth exists.  Every disjoint row gets the comparison.
        assert np.array_equal(use, np.asarray(ex["gap"] > 0)) and use.mean() > 0.45
    elif cs["family"] in "TA":
        assert use.mean() >= SHARE, (name, float(use.mean()))
    else:
        assert not use.any() or name == "C sphere centre on box face"
    closed = cs["closed"]
    has = np.isfinite(closed)
    if has.any():  # the closed-form depths of family C
        assert np.abs(ex["E"][rows, col][has] - closed[has]).max() <= AGREE, name
