"""Per-model specialised filter kernels.

``mjpl_create`` compiles a model into a *program* -- control words ``ip`` and constant tables
``fp`` / ``dp`` -- which the generic kernels of ``mjpl_device.h`` interpret: every body, joint, geom
and four-row chunk of partners costs scalar loads of control words, address arithmetic, loop
branches and mask bookkeeping (0.78 scalar instructions per vector instruction in the item pass,
round-1 counters).  This module turns ONE program into straight-line HIP source instead:

* forward kinematics with the model's constants as literals, terms that multiply an exact 0
  dropped and exact +-1 folded at generation time (a hinge about z contributes two products per
  quaternion component instead of four);
* one bounding cull per ENABLED partner, operands as literals, each hit mask parked in lane k of a
  register pair (``v_writelane``) so that one rolled loop per geom -- the only copy of the push and
  drain code -- picks the partners some lane passed (``ballot`` of the non-zero lanes);
* the candidate queues, the drains (full-lane narrowphase), the exact re-check of undecided pairs
  and every table they read are the generic ones: verdicts are the same.

The generated code is compiled with the kernels of ``mjpl_filter.h`` into
``mjpl_amd/csrc/spec/libmjpl_spec_<hash>.so``; an engine whose program has that hash loads it
(``mjpl_hip.hip: load_spec``).  Building needs ``hipcc`` and no GPU (``mjpl_program_dump`` compiles
the model on the host), so it runs in the build container, or on a GPU box BEFORE the process
touches the GPU.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
import os
import subprocess
import threading
from typing import NamedTuple

import numpy as np

from . import build as _build
from . import engine as _engine
from .engine import _ptr
from .fold import Fold, dlit
# (the layout constants stay names of this module: tools and tests walk the layout through them)
from .program import (B_BODYID, B_DOFF, B_NGEOM, B_NJNT, B_PARENT, B_SAVE, B_SIZE, EK_PLANE, EK_SLOT, EK_STATIC, FC_MAXANGLE,  # noqa: F401
                      FC_MAXCOORD, G_DOFF, G_FLAGS, G_GEOMID, G_PMASK_HI, G_PMASK_LO, G_SIZE, G_SMASK, G_STORE, G_TYPE, G_WMASK_HI,
                      G_WMASK_LO, GD_SIZE, GD_WBOUND, GF_SAMEPOS, GF_SAMEROT, GT_BOX, GT_CAPSULE, GT_PLANE, GT_SPHERE, H_NBODYOPS,
                      H_NPLAN, H_NSAVE, H_NSLOTS, H_NWORLD, H_NWPAD, H_OFF_BODYOPS, H_OFF_FCONST, H_OFF_PERM, H_OFF_WCULL,
                      H_OFF_WNARROW, H_SIZE, J_DOFF, J_FLAGS, J_QSRC, J_SIZE, J_TYPE, JF_POS_NONZERO, JT_HINGE, JT_SLIDE, MAX_SLOTS,
                      P_FIRST, PARENT_CUR, PARENT_STATIC, SLOT_NONE, WN_LEN, WN_ZAXIS, Geom, decode)

SPEC_DIR = os.path.join(_build.CSRC, "spec")
# under SPEC_DIR: a few libraries once more WITHOUT build.codegen_flags' option (build(uniform_regions=False)), compiled by
# __graft_entry__.build() and compared bit for bit by tests/test_gpu_uniform_regions.py
STRUCTURIZED_SUBDIR = "structurized"
# ... and once more with the pose arithmetic as plain expressions and sincosf (build(opts=Options.for_build()._replace(
# pose_fma=False, sincos=False))): the text without the helpers of mjpl_pose_f32.h, compared by tests/test_gpu_pose_fma.py
UNFUSED_SUBDIR = "unfused"


class ProgramInfo(C.Structure):
    _fields_ = [("hash", C.c_uint64), ("maxs", C.c_int32), ("wbox", C.c_int32), ("mbox", C.c_int32),
                ("immediate", C.c_int32), ("filter_usable", C.c_int32), ("filter_tol", C.c_float),
                ("nslots", C.c_int32), ("nsave", C.c_int32), ("spec_abi", C.c_int32),
                ("robot_hash", C.c_uint64), ("scene_rows", C.c_int32), ("scene_ok", C.c_int32)]


def _dump(model, allowed_collision_bodies, qidx, qpos_base, filter_tol, prune_pairs):
    """mjpl_program_dump (prune_pairs None) or mjpl_program_dump_pruned -> (ip, fp, dp, ProgramInfo, dropped int32 [n, 2])."""
    lib = _engine.load_library()
    head, keep = _engine._compile_args(model, allowed_collision_bodies, qidx, qpos_base)
    info = ProgramInfo()
    nip, ntab, ndrop = C.c_int32(0), C.c_int32(0), C.c_int32(0)

    def args(bufs):
        ip, fp, dp, dropped = bufs or (None, None, None, None)
        ndrop.value = 0 if dropped is None else len(dropped)
        tables = [_ptr(ip, _engine._I32P), C.byref(nip), _ptr(fp, C.POINTER(C.c_float)), _ptr(dp, _engine._F64P), C.byref(ntab), C.byref(info)]
        if prune_pairs is None:
            return [*head, C.c_double(filter_tol), *tables]
        return [*head, C.c_double(filter_tol), C.c_int32(int(prune_pairs)), *tables, _ptr(dropped, _engine._I32P), C.byref(ndrop)]

    def alloc(_):
        return np.zeros(nip.value, np.int32), np.zeros(ntab.value, np.float32), np.zeros(ntab.value, np.float64), np.zeros((ndrop.value, 2), np.int32)
    ip, fp, dp, dropped = _engine._sized_call(lib, lib.mjpl_program_dump if prune_pairs is None else lib.mjpl_program_dump_pruned, args, alloc)
    return ip, fp, dp, info, dropped


def dump_program(model, allowed_collision_bodies=(), qidx=None, qpos_base=None, filter_tol: float = 0.0):
    """Compile `model` on the host (no GPU) -> (ip int32[], fp float32[], dp float64[], ProgramInfo): the program an
    engine runs by default."""
    return _dump(model, allowed_collision_bodies, qidx, qpos_base, filter_tol, None)[:4]


def dump_program_pruned(model, allowed_collision_bodies=(), qidx=None, qpos_base=None, filter_tol: float = 0.0, prune_pairs: int = 1):
    """dump_program with the option "prune_pairs" forced (0: every enabled pair stays in the program, 1: the default, 2: self
    pairs are dropped as well) -> (ip, fp, dp, ProgramInfo, dropped): dropped = the geom pairs the program leaves out,
    int32 [n, 2], g1 < g2."""
    return _dump(model, allowed_collision_bodies, qidx, qpos_base, filter_tol, int(prune_pairs))


def dump_never_touch(model, allowed_collision_bodies=(), qidx=None, qpos_base=None, filter_tol: float = 0.0, prune_pairs: int = 1,
                     prune_contacts: int = 1):
    """The side set of the program dump_program_pruned(..., prune_pairs) compiles (mjpl_program_dump_never_touch; DESIGN.md
    5.1d) -> (pairs int32 [n, 2] with g1 < g2, cell evaluations spent, program hash, hash of ip / fp / dp alone): enabled pairs of a moving geom with a
    static geom or a plane proved never to come within their contact margin.  ip / fp / dp keep them; `generate` leaves
    them out of a per-program library.  prune_contacts: 0 the empty set, 1 the default, >= 2 that many cell evaluations per
    pair at most (tests)."""
    lib = _engine.load_library()
    head, keep = _engine._compile_args(model, allowed_collision_bodies, qidx, qpos_base)
    n, evals, h, th = C.c_int32(0), C.c_int32(0), C.c_uint64(0), C.c_uint64(0)

    def args(pairs):
        n.value = 0 if pairs is None else len(pairs)
        return [*head, C.c_double(filter_tol), C.c_int32(int(prune_pairs)), C.c_int32(int(prune_contacts)), _ptr(pairs, _engine._I32P),
                C.byref(n), C.byref(evals), C.byref(h), C.byref(th)]
    pairs = _engine._sized_call(lib, lib.mjpl_program_dump_never_touch, args, lambda _: np.zeros((n.value, 2), np.int32))
    return pairs, int(evals.value), int(h.value), int(th.value)


# ----------------------------------------------------------------------------- expression helpers
def lit(x: float) -> str:
    """Exact C literal of a binary32 value."""
    x = float(np.float32(x))
    if math.isnan(x):
        return "__builtin_nanf(\"\")"
    if math.isinf(x):
        return "__builtin_inff()" if x > 0 else "(-__builtin_inff())"
    return f"{x.hex()}f"


def lin(terms, const: float = 0.0) -> str:
    """sum of coef * expr with exact-zero terms dropped and exact +-1 coefficients folded;
    `terms` = [(coef, expr)].  Returns a C expression (float)."""
    parts = []
    for c, e in terms:
        c = float(np.float32(c))
        if c == 0.0:
            continue
        if c == 1.0:
            parts.append(("+", e))
        elif c == -1.0:
            parts.append(("-", e))
        elif c < 0:
            parts.append(("-", f"{lit(-c)} * {e}"))
        else:
            parts.append(("+", f"{lit(c)} * {e}"))
    const = float(np.float32(const))
    if const != 0.0:
        parts.append(("+" if const > 0 else "-", lit(abs(const))))
    if not parts:
        return "0.0f"
    out = ("-" if parts[0][0] == "-" else "") + parts[0][1]
    for sgn, e in parts[1:]:
        out += f" {sgn} {e}"
    return f"({out})"


def quat_mul_const_right(a, b) -> list[str]:
    """a (expressions) x b (constants) -> 4 expressions (mju_mulQuat)."""
    return [lin([(b[0], a[0]), (-b[1], a[1]), (-b[2], a[2]), (-b[3], a[3])]),
            lin([(b[1], a[0]), (b[0], a[1]), (b[3], a[2]), (-b[2], a[3])]),
            lin([(b[2], a[0]), (-b[3], a[1]), (b[0], a[2]), (b[1], a[3])]),
            lin([(b[3], a[0]), (b[2], a[1]), (-b[1], a[2]), (b[0], a[3])])]


def flin(terms, base: str | None = None) -> str:
    """lin() with fused multiply-adds: the sum of coef * expr (onto `base`, if given) as one chain of __builtin_fmaf in the
    order of `terms` -- the association of mjpl::pose_mul_quat and its kin (mjpl_pose_f32.h) -- with exact-zero terms
    dropped and exact +-1 coefficients folded into an addition."""
    acc = base
    for c, e in terms:
        c = float(np.float32(c))
        if c == 0.0:
            continue
        if acc is None:
            acc = e if c == 1.0 else (f"(-{e})" if c == -1.0 else f"({lit(c)} * {e})")
        elif c == 1.0:
            acc = f"({acc} + {e})"
        elif c == -1.0:
            acc = f"({acc} - {e})"
        else:
            acc = f"__builtin_fmaf({lit(c)}, {e}, {acc})"
    return "0.0f" if acc is None else acc


def _general(coefs) -> bool:
    """No coefficient folds (none is an exact 0 or +-1 in binary32): the statement is a call of the header's helper."""
    return all(float(np.float32(c)) not in (0.0, 1.0, -1.0) for c in coefs)


def quat_mul_const_right_fused(a, b) -> list[str]:
    """quat_mul_const_right as chains of fused multiply-adds: term for term mjpl::pose_mul_quat."""
    return [flin([(b[0], a[0]), (-b[1], a[1]), (-b[2], a[2]), (-b[3], a[3])]),
            flin([(b[1], a[0]), (b[0], a[1]), (b[3], a[2]), (-b[2], a[3])]),
            flin([(b[2], a[0]), (-b[3], a[1]), (b[0], a[2]), (b[1], a[3])]),
            flin([(b[3], a[0]), (b[2], a[1]), (-b[1], a[2]), (b[0], a[3])])]


def quat_mul_np(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def expanded_threshold(X, bound, reach: float) -> float:
    """Threshold of the expanded bounding cull of a static partner at X (binary32 coordinates) whose
    difference-form bound is `bound` (already widened by the filter's tolerance): the test
        fl(|c|^2 - 2 c.X) <= THR
    must pass whenever the real-arithmetic |c - X|^2 <= bound for a centre c with |c| <= reach.
    |c|^2 costs three roundings of at most u |c|^2 (u = 2^-24), each of the three multiply-adds one of at
    most u (|c| + |X|)^2 (every partial sum is bounded by that): the computed value exceeds the real one by
    no more than 6 u (|c| + |X|)^2.  The allowance below takes 8 u, a reach larger by one percent, and the
    threshold is rounded up to binary32."""
    X = np.asarray([float(np.float32(v)) for v in X], dtype=np.float64)
    nx = float(np.linalg.norm(X))
    b = float(np.float32(bound))
    if not math.isfinite(b):
        return b
    if not math.isfinite(reach):
        return math.inf  # (nothing bounds the centre: every lane is a candidate; the narrowphase decides)
    allow = 8.0 * 2.0 ** -24 * (1.01 * reach + nx) ** 2
    thr = b - float(X @ X) + allow
    f = np.float32(thr)
    if float(f) < thr:
        f = np.nextafter(f, np.float32(np.inf))
    return float(f)


class Options(NamedTuple):
    """The generation switches.  The environment is their outside interface: the public entry points (generate,
    generate_full_exact, translation_unit, build) read it once, here, and pass the value down."""
    cull: str = "expanded"     # MJPL_SPEC_CULL: the form of the static culls (see generate)
    cert: bool = False         # MJPL_SPEC_CERT=1: the edge certificate, where the program admits one
    f64: bool = False          # MJPL_SPEC_F64=1: libraries carry the generated float64 check (generate_full_exact)
    f64_inline: bool = False   # MJPL_SPEC_F64_INLINE=1: ... inlined, for tools/f64_inline_probe.py
    mbox_waves: int = 2        # MJPL_SPEC_MBOX_WAVES: waves per SIMD the kernels of a model with moving boxes are built for (A/B builds)
    # The two switches of the fused pose text (mjpl_pose_f32.h).  Off, the generator writes the plain expressions it always
    # wrote -- the text tests/golden/generated_source_digests.json records; build() turns pose_fma on (for_build), so every
    # library it compiles on its own carries the fused arithmetic; MJPL_SPEC_POSE_FMA=0 / MJPL_SPEC_SINCOS=1 there, or
    # build(opts=...), give the comparison libraries of the A/B.
    pose_fma: bool = False     # MJPL_SPEC_POSE_FMA: the pose arithmetic as calls of mjpl::pose_* (fused multiply-adds in a fixed order)
    sincos: bool = False       # MJPL_SPEC_SINCOS: a hinge's half angle through mjpl::sincos_half_f32, not sincosf

    @classmethod
    def from_env(cls) -> "Options":
        e = os.environ.get
        return cls(e("MJPL_SPEC_CULL", "expanded"), e("MJPL_SPEC_CERT", "0") == "1", e("MJPL_SPEC_F64") == "1",
                   e("MJPL_SPEC_F64_INLINE") == "1", max(1, min(3, int(e("MJPL_SPEC_MBOX_WAVES", "2")))),
                   e("MJPL_SPEC_POSE_FMA") == "1", e("MJPL_SPEC_SINCOS") == "1")

    @classmethod
    def for_build(cls) -> "Options":
        """What build() generates with when its caller passes no switches: the environment's, with the fused pose arithmetic
        on unless the environment says 0.  sincos stays an opt-in (MJPL_SPEC_SINCOS=1): measured alone it does not pay -- its
        665 fewer vector instructions cost four more spilled registers (profiles/README.md, r12)."""
        return cls.from_env()._replace(pose_fma=os.environ.get("MJPL_SPEC_POSE_FMA", "1") != "0")


class _Gen:
    def __init__(self, opts: Options = Options()):
        self.lines: list[str] = []
        self.pose_fma, self.sincos = opts.pose_fma, opts.sincos

    def w(self, s="", ind=3):
        self.lines.append("  " * ind + s)

    # rot_vec_quat(res, const vec, quat expr): v + 2 * cross(q_xyz, q_w v + cross(q_xyz, v))
    def rot_vec_quat(self, dst, vec, qn):
        v = [float(x) for x in vec]
        if self.pose_fma and _general(v):
            self.w(f"{{ const float v_[3] = {{{lit(v[0])}, {lit(v[1])}, {lit(v[2])}}}, q_[4] = {{{qn[0]}, {qn[1]}, {qn[2]}, {qn[3]}}};")
            self.w(f"  float r_[3]; mjpl::pose_rot_vec(r_, v_, q_); {dst}0 = r_[0]; {dst}1 = r_[1]; {dst}2 = r_[2]; }}")
            return
        if self.pose_fma:  # (some component folds: the chains of mjpl::pose_rot_vec with those terms dropped)
            self.w(f"{{ const float t0_ = {flin([(v[0], qn[0]), (v[2], qn[2]), (-v[1], qn[3])])};")
            self.w(f"  const float t1_ = {flin([(v[1], qn[0]), (v[0], qn[3]), (-v[2], qn[1])])};")
            self.w(f"  const float t2_ = {flin([(v[2], qn[0]), (v[1], qn[1]), (-v[0], qn[2])])};")
            self.w(f"  {dst}0 = __builtin_fmaf(2.0f, __builtin_fmaf({qn[2]}, t2_, -({qn[3]} * t1_)), {lit(v[0])});")
            self.w(f"  {dst}1 = __builtin_fmaf(2.0f, __builtin_fmaf({qn[3]}, t0_, -({qn[1]} * t2_)), {lit(v[1])});")
            self.w(f"  {dst}2 = __builtin_fmaf(2.0f, __builtin_fmaf({qn[1]}, t1_, -({qn[2]} * t0_)), {lit(v[2])}); }}")
            return
        self.w(f"{{ const float t0_ = {lin([(v[0], qn[0]), (v[2], qn[2]), (-v[1], qn[3])])};")
        self.w(f"  const float t1_ = {lin([(v[1], qn[0]), (v[0], qn[3]), (-v[2], qn[1])])};")
        self.w(f"  const float t2_ = {lin([(v[2], qn[0]), (v[1], qn[1]), (-v[0], qn[2])])};")
        self.w(f"  {dst}0 = {lit(v[0])} + 2.0f * ({qn[2]} * t2_ - {qn[3]} * t1_);")
        self.w(f"  {dst}1 = {lit(v[1])} + 2.0f * ({qn[3]} * t0_ - {qn[1]} * t2_);")
        self.w(f"  {dst}2 = {lit(v[2])} + 2.0f * ({qn[1]} * t1_ - {qn[2]} * t0_); }}")


SCENE_ROWS, SCENE_HEADER, SCENE_SLOT_LANE0 = 32, 32, 40  # (mjpl_filter.h: kSceneRows, kSceneHeader)
SCENE_PLANE_ROWS, SCENE_STAGE = 2, 32 * 4 + 32              # (kScenePlaneRows, kSceneStageFloats)


def pack_desc(kind, index, ptype, pfirst, boxq, index2=0, lvl=0) -> int:
    """The descriptor of one partner of a stage (kSpecDesc / kExactDesc): what the rolled push loop reads per hit."""
    return (kind << 0) | (index << 2) | (ptype << 10) | (pfirst << 14) | (boxq << 15) | (index2 << 16) | (lvl << 22)


# ----------------------------------------------------------------------------- analyses of a decoded program (no text)
def _along_chain(prog, init, root, step) -> list:
    """One value per body op, handed down the tree the way the poses are: step(body, the parent's value) with the parent
    the body before (PARENT_CUR; `init` in front of the first), a static one (root(body)) or a saved one."""
    cur, saved, out = init, {}, []
    for b in prog.bodies:
        cur = step(b, root(b) if b.parent == PARENT_STATIC else (cur if b.parent == PARENT_CUR else saved[b.parent - 1]))
        out.append(cur)
        if b.save >= 0:
            saved[b.save] = cur
    return out


def _body_reach(prog, fp, dp) -> list:
    """How far from the world origin can a moving geom's centre be while its lane is still alive?  Per body op: the body
    origins by the triangle inequality along the chain (hinges keep lengths; an off-centre hinge adds
    twice its offset), or -- below a slide joint, whose travel the program does not know -- by the
    per-lane range check: a lane whose body origin leaves [-maxcoord, maxcoord]^3 is dead from there on."""
    box_reach = math.sqrt(3.0) * float(fp[prog.off_fconst + FC_MAXCOORD])

    def step(b, parent_reach):
        reach = parent_reach + float(np.linalg.norm(dp[b.doff: b.doff + 3]))
        for j in b.joints:
            reach = math.inf if j.type == JT_SLIDE else reach + 2.0 * float(np.linalg.norm(dp[j.doff + 3: j.doff + 6]))
        return min(reach, box_reach)
    return _along_chain(prog, 0.0, lambda b: float(np.linalg.norm(dp[b.doff + 7: b.doff + 10])), step)


def _body_levers(prog, dp) -> tuple:
    """The edge certificate (mjpl_fused.h): how far can any point of a moving geom travel while the
    planning joints go from one end of an edge to the other?  At most  sum_j |dq_j| rho_j  over the planning hinges j
    above it, rho_j = the longest the chain can stretch from joint j's anchor to the geom's centre + the geom's
    bounding radius (hinges keep lengths: a triangle inequality along the chain, as `_body_reach`).
    -> (per body op `anc`: [(planning column, that length up to the body's origin)] root first, False where a planning
    SLIDE joint rules the certificate out)."""
    ok = True

    def step(b, anc_parent):
        nonlocal ok
        blen = float(np.linalg.norm(dp[b.doff: b.doff + 3]))
        anc = [(qs, d + blen) for qs, d in anc_parent]
        for j in b.joints:
            jp = float(np.linalg.norm(dp[j.doff + 3: j.doff + 6]))
            if j.type == JT_SLIDE:
                if j.qsrc >= 0:
                    ok = False
                else:  # a slide joint held at its constant: a fixed offset along its axis
                    off = abs(float(dp[j.doff + 7]) - float(dp[j.doff + 6]))
                    anc = [(qs, d + off) for qs, d in anc]
            else:
                anc = [(qs, d + 2.0 * jp) for qs, d in anc]
                if j.qsrc >= 0:
                    anc.append((j.qsrc, jp))
        return anc
    return _along_chain(prog, [], lambda b: [], step), ok


def _slot_levels(prog, anc, maxs) -> tuple:
    """Per stage {slot: certificate level of the geom stored there}: the planning joints above a stored geom must be a
    prefix of those above the geom tested against it, and at most 7 -- the level is their number (0: relative to the
    world).  -> (levels, False where some moving pair does not nest so: level 0 there, and no certificate)."""
    slot_anc, out, ok = {}, [], True   # slot -> planning columns above the geom stored there
    for g in prog.geoms:
        mine, lv = [qs for qs, _ in anc[g.body]], {}
        for n, _ in g.slots(maxs):
            theirs = slot_anc.get(n)
            nested = theirs is not None and mine[:len(theirs)] == theirs and len(theirs) <= 7
            ok, lv[n] = ok and nested, len(theirs) if nested else 0
        out.append(lv)
        if g.store >= 0:
            slot_anc[g.slot] = mine
    return out, ok


def _axes_slots(prog, dp, mbox: bool, share: bool, statics: list):
    """Moving boxes: boxes of one body with one orientation (the Panda's five pads per finger) have ONE frame --
    the x and y axes are kept once, in the second slot of the first of them.  Per stage (`axes_of` at its culls: each
    stored box's own second slot -> the slot that holds the values, the slot this geom stores its axes in or 63).
    None: the program's own slot allocation reuses a shared slot while boxes still refer to it (never without sharing).
    statics: the static partners per stage (_world_partners).  The generator has always named a frame's owner by the last
    static partner its body's geoms so far tested in a pair of two, where there is one, and by the body otherwise: two boxes
    of a body share only where that partner (lane, centre, bound) is the same, which is less often than they could.
    Kept, because generated text follows from it."""
    axes_of: dict[int, int] = {}
    axes_key: dict[int, tuple] = {}   # whose axes a slot holds right now
    out = []

    def referred(slot):
        return any(v == slot and k != v for k, v in axes_of.items())
    owner = None
    for g in prog.geoms:
        if g.stage == prog.bodies[g.body].geoms[0].stage:  # (the first geom of its body)
            owner = g.body
        if len(statics[g.stage]) >= 2:
            owner = statics[g.stage][len(statics[g.stage]) // 2 * 2 - 1]
        at_culls = dict(axes_of)
        store2 = ((g.store >> 6) & 63) if (g.store >= 0 and mbox) else 63
        if g.store >= 0 and g.slot in axes_key:  # (a slot that held shared axes is written again: nobody may still read them)
            if referred(g.slot):
                return None
            del axes_key[g.slot]
        if store2 != 63:
            key = (owner, bool(g.flags & GF_SAMEROT), tuple(np.float32(dp[g.doff + 3: g.doff + 7]).tolist()))
            held = [sl for sl, k_ in axes_key.items() if k_ == key] if share else []
            if held:           # the frame is in the slot file already
                axes_of[store2] = held[0]
                store2 = 63
            else:
                if referred(store2):
                    return None
                axes_of[store2] = store2
                axes_key[store2] = key
        out.append((at_culls, store2))
    return out


class _Stage(NamedTuple):
    """One moving geom with the partners its bounding sphere is tested against; k: the lane its hit mask is parked in."""
    geom: Geom
    curbox: bool    # a moving box: the whole frame is kept
    planes: list    # [(k, world row, bound)]
    statics: list   # [(k, X, Y, Z, bound)]
    slots: list     # [(k, slot, bound, certificate level)]
    desc: list      # the packed descriptors, lane by lane
    reach: float    # how far from the origin the centre can be (_body_reach + the geom's offset)
    store2: int     # slot its x and y axes are stored in, or 63


def _world_partners(prog, g, fp, info, generic, skip) -> tuple:
    """The static partners of moving geom g -> (planes, statics, their descriptors: see _Stage), without the never-touch
    pairs `skip`; none in a scene-generic library, where they are rows of the scene table."""
    curbox = bool(info.mbox) and g.type == GT_BOX
    wbound = fp[g.doff + GD_WBOUND:]
    planes, statics, desc = [], [], []
    for wrow in ([] if generic else g.world_rows(planes=True)):
        pgid = prog.row_info(fp, wrow)[1]
        if (min(g.geom_id, pgid), max(g.geom_id, pgid)) in skip:
            continue
        planes.append((len(desc), wrow, wbound[wrow]))
        desc.append(pack_desc(EK_PLANE, wrow, GT_PLANE, 1, 1 if curbox else 0, 63))
    for wrow in ([] if generic else g.world_rows(planes=False)):
        ptype, pgid = prog.row_info(fp, wrow)
        if (min(g.geom_id, pgid), max(g.geom_id, pgid)) in skip:
            continue
        pfirst = 1 if (ptype < g.type or (ptype == g.type and pgid < g.geom_id)) else 0
        statics.append((len(desc), *(float(fp[prog.wc_at(wrow, f)]) for f in range(3)), wbound[wrow]))
        desc.append(pack_desc(EK_STATIC, wrow, ptype, pfirst, 1 if (ptype == GT_BOX or curbox) else 0, 63))
    return planes, statics, desc


def _partners(prog, g, fp, dp, info, generic, world, levels, axes, body_reach) -> _Stage:
    """The partner list of moving geom g: its static partners `world`, then the earlier moving geoms in the slot file
    (from lane 40 on in a scene-generic library)."""
    mbox = bool(info.mbox)  # moving boxes: full frames in the box queue, two register slots per stored box
    curbox = mbox and g.type == GT_BOX
    sbound = fp[g.doff + GD_WBOUND + 2 * prog.nwpad:]
    (planes, statics, desc), slots = world, []
    axes_of, store2 = axes
    for n, pw in g.slots(int(info.maxs)):
        if generic:  # (lanes 0 .. 31 belong to the scene rows)
            desc += [0] * (SCENE_SLOT_LANE0 - len(desc))
        sptype = (pw >> 12) & 15
        # (a stored box keeps its x and y axes in a second slot, pw & 63; with a box on either side the pair
        # takes the box queue, whose records carry full frames)
        n2 = (pw & 63) if mbox else 63
        if n2 != 63:
            n2 = axes_of[n2]
        slots.append((len(desc), n, sbound[n], levels[n]))
        desc.append(pack_desc(EK_SLOT, n, sptype, 1 if (pw & P_FIRST) else 0, 1 if (mbox and (curbox or sptype == GT_BOX)) else 0, n2, levels[n]))
    if len(desc) > 64:
        raise ValueError("a geom with more than 64 enabled partners cannot be specialised")
    reach = body_reach + float(np.linalg.norm(np.asarray(dp[g.doff: g.doff + 3], dtype=np.float64)))
    return _Stage(g, curbox, planes, statics, slots, desc, reach, store2)


def _certificate(st: _Stage, dp, anc) -> tuple:
    """The certificate block of a stage: suffix sums of |dq_j| rho_j from the deepest planning joint up; level c =
    the motion relative to a geom that hangs on the first c of them (0: to the world).
    -> (False where the geom has no bounding radius or more than 7 planning joints above it, the block's lines,
    (geom id, [(planning column, rho)], bounding radius): an entry of report["cert_levers"])."""
    g = st.geom
    sizes = [float(x) for x in dp[g.doff + GD_SIZE: g.doff + GD_SIZE + 3]]
    rbound = {GT_SPHERE: sizes[0], GT_CAPSULE: sizes[0] + sizes[1], GT_BOX: math.sqrt(sum(x * x for x in sizes))}.get(g.type, math.inf)
    lp = float(np.linalg.norm(np.asarray(dp[g.doff: g.doff + 3], dtype=np.float64)))
    levers = [(qs, d + lp + (rbound if math.isfinite(rbound) else 0.0)) for qs, d in anc]
    k2w = max([2.0 * math.sqrt(max(float(bound), 0.0)) for _, _, _, _, bound in st.statics] + [0.0])
    slot_k2 = max([2.0 * math.sqrt(max(float(bound), 0.0)) for _, _, bound, _ in st.slots] + [0.0])
    slot_levels = {lvl for _, _, _, lvl in st.slots}
    cb = ["float s_ = 0.0f;"]
    for lv in range(len(anc), -1, -1):
        if lv < len(anc):
            cb.append(f"s_ = __builtin_fmaf((float)adq[{levers[lv][0]} * 64], {lit(levers[lv][1] * (1.0 + 1e-6))}, s_);")
        if lv in slot_levels | {0}:
            cb.append(f"dm{lv} = __builtin_fmaf(s_, 1.001f, 2.0f * tol);")
    cb.append(f"wc0 = __builtin_fmaf({lit(k2w * (1.0 + 1e-6))}, dm0, dm0 * dm0); deadp = dead - dm0;")
    for lv in sorted(slot_levels):
        cb.append(f"ws{lv} = __builtin_fmaf({lit(slot_k2 * (1.0 + 1e-6))}, dm{lv}, dm{lv} * dm{lv});")
    return math.isfinite(rbound) and len(anc) <= 7, cb, (g.geom_id, levers, rbound)


# ----------------------------------------------------------------------------- emitters (text from analysed data)
def _lin3(g: _Gen, base: str, c, r: int) -> str:
    """base + c . (row r of the rotation matrix R0 .. R8), c literal: a body's origin, a geom's centre."""
    terms = [(c[k], f"R{3 * r + k}") for k in range(3)]
    if not g.pose_fma:
        return f"{base} + {lin(terms)}"
    if _general(c):
        return f"mjpl::pose_lin3({base}, {', '.join(f'{lit(ck)}, {e}' for ck, e in terms)})"
    left = [t for t in terms if float(np.float32(t[0])) != 0.0]
    if len(left) <= 1:  # (one multiply-add onto the world coordinate: its one rounding at that magnitude)
        return flin(left, base)
    return f"({base} + {flin(left)})"  # (as pose_lin3: the products summed first, the world coordinate added once)


def _emit_quat_mul_const(g: _Gen, typ: str, dst: str, b):
    """`typ` {dst}0 .. {dst}3 = (q0, q1, q2, q3) (x) the literal quaternion b."""
    qn = ["q0", "q1", "q2", "q3"]
    if g.pose_fma and _general(b):
        g.w(f"float {dst}0, {dst}1, {dst}2, {dst}3;")
        g.w(f"{{ const float a_[4] = {{q0, q1, q2, q3}}, b_[4] = {{{', '.join(lit(x) for x in b)}}}; float r_[4];")
        g.w(f"  mjpl::pose_mul_quat(r_, a_, b_); {dst}0 = r_[0]; {dst}1 = r_[1]; {dst}2 = r_[2]; {dst}3 = r_[3]; }}")
        return
    e = quat_mul_const_right_fused(qn, b) if g.pose_fma else quat_mul_const_right(qn, b)
    g.w(f"{typ} {dst}0 = {e[0]}, {dst}1 = {e[1]}, {dst}2 = {e[2]}, {dst}3 = {e[3]};")


def _emit_body_fk(g: _Gen, body, dp):
    """Forward kinematics of one body op: the parent's pose, the joints, normalisation, range check, save."""
    w = g.w
    bd = dp[body.doff:]
    if body.parent == PARENT_STATIC:
        pp, pq, pR = bd[7:10].copy(), bd[10:14].copy(), bd[14:23].copy()
        npc = pp + pR.reshape(3, 3) @ bd[0:3]
        nqc = quat_mul_np(pq, bd[3:7])
        w(f"float np0 = {lit(npc[0])}, np1 = {lit(npc[1])}, np2 = {lit(npc[2])};")
        w(f"float nq0 = {lit(nqc[0])}, nq1 = {lit(nqc[1])}, nq2 = {lit(nqc[2])}, nq3 = {lit(nqc[3])};")
    else:
        if body.parent != PARENT_CUR:  # restore a saved pose
            w(f"{{ const float *sv = save + (size_t){body.parent - 1} * 7 * sstride;")
            w("  p0 = sv[0]; p1 = sv[sstride]; p2 = sv[2 * sstride];")
            w("  q0 = sv[3 * sstride]; q1 = sv[4 * sstride]; q2 = sv[5 * sstride]; q3 = sv[6 * sstride];")
            w("  MJPL_SPEC_QUAT2MAT(); }")
        bp, bq = bd[0:3], bd[3:7]
        for r in range(3):
            w(f"float np{r} = {_lin3(g, f'p{r}', bp, r)};")
        _emit_quat_mul_const(g, "float", "nq", bq)
    for jtype, qsrc, jflags, jdoff in body.joints:
        jd = dp[jdoff:]
        axis, jpos, qpos0, qconst = jd[0:3], jd[3:6], float(jd[6]), float(jd[7])
        if qsrc >= 0:
            w(f"{{ const float dq = (float)q[{qsrc} * qstride] - {lit(qpos0)};")
        else:
            w(f"{{ const float dq = {lit(np.float32(qconst) - np.float32(qpos0))};")
        nqn = ["nq0", "nq1", "nq2", "nq3"]
        if jtype == JT_SLIDE:
            w("  float xa0, xa1, xa2;")
            g.rot_vec_quat("xa", axis, nqn)
            if g.pose_fma:
                w("  np0 = __builtin_fmaf(xa0, dq, np0); np1 = __builtin_fmaf(xa1, dq, np1); np2 = __builtin_fmaf(xa2, dq, np2); }")
            else:
                w("  np0 += xa0 * dq; np1 += xa1 * dq; np2 += xa2 * dq; }")
        else:
            if jflags & JF_POS_NONZERO:
                w("  float an0, an1, an2;")
                g.rot_vec_quat("an", jpos, nqn)
                w("  an0 += np0; an1 += np1; an2 += np2;")
            w("  far = far || !(fabsf(dq) <= maxangle);  // binary32(q) is off by eps |q|")
            w(f"  float sn, cs; {'mjpl::sincos_half_f32' if g.sincos else 'sincosf'}(dq * 0.5f, &sn, &cs);")
            # nq = nq (x) (cs, ax sn, ay sn, az sn)
            a = [float(np.float32(x)) for x in axis]
            if g.pose_fma and _general(a):
                w(f"  {{ const float ax_[3] = {{{lit(a[0])}, {lit(a[1])}, {lit(a[2])}}}; float h_[4] = {{nq0, nq1, nq2, nq3}};")
                w("    mjpl::pose_hinge(h_, ax_, sn, cs); nq0 = h_[0]; nq1 = h_[1]; nq2 = h_[2]; nq3 = h_[3]; }")
            elif g.pose_fma:  # (some component of the axis folds: the chains of mjpl::pose_hinge with those terms dropped)
                sx = [None if a[k] == 0.0 else ("sn" if a[k] == 1.0 else ("(-sn)" if a[k] == -1.0 else f"({lit(a[k])} * sn)")) for k in range(3)]
                rows = [[(1, "nq0", "cs"), (-1, "nq1", sx[0]), (-1, "nq2", sx[1]), (-1, "nq3", sx[2])],
                        [(1, "nq0", sx[0]), (1, "nq1", "cs"), (1, "nq2", sx[2]), (-1, "nq3", sx[1])],
                        [(1, "nq0", sx[1]), (-1, "nq1", sx[2]), (1, "nq2", "cs"), (1, "nq3", sx[0])],
                        [(1, "nq0", sx[2]), (1, "nq1", sx[1]), (-1, "nq2", sx[0]), (1, "nq3", "cs")]]
                exprs = []
                for row in rows:
                    acc = None
                    for sign, left, right in row:
                        if right is None:
                            continue
                        left = left if sign > 0 else f"-{left}"
                        acc = f"{left} * {right}" if acc is None else f"__builtin_fmaf({left}, {right}, {acc})"
                    exprs.append(acc)
                w(f"  const float t0 = {exprs[0]}, t1 = {exprs[1]}, t2 = {exprs[2]}, t3 = {exprs[3]};")
                w("  nq0 = t0; nq1 = t1; nq2 = t2; nq3 = t3;")
            else:
                sx = [f"{lit(a[k])} * sn" if a[k] not in (0.0, 1.0, -1.0) else ("sn" if a[k] == 1.0 else ("(-sn)" if a[k] == -1.0 else None))
                      for k in range(3)]

                def term(sign, left, right):
                    return None if right is None else (sign, f"{left} * {right}")

                comps = [
                    [("+", "nq0 * cs"), term("-", "nq1", sx[0]), term("-", "nq2", sx[1]), term("-", "nq3", sx[2])],
                    [term("+", "nq0", sx[0]), ("+", "nq1 * cs"), term("+", "nq2", sx[2]), term("-", "nq3", sx[1])],
                    [term("+", "nq0", sx[1]), term("-", "nq1", sx[2]), ("+", "nq2 * cs"), term("+", "nq3", sx[0])],
                    [term("+", "nq0", sx[2]), term("+", "nq1", sx[1]), term("-", "nq2", sx[0]), ("+", "nq3 * cs")],
                ]
                exprs = []
                for comp in comps:
                    ts = [t for t in comp if t is not None]
                    out = ("-" if ts[0][0] == "-" else "") + ts[0][1]
                    for sgn, ex in ts[1:]:
                        out += f" {sgn} {ex}"
                    exprs.append(out)
                w(f"  const float t0 = {exprs[0]}, t1 = {exprs[1]}, t2 = {exprs[2]}, t3 = {exprs[3]};")
                w("  nq0 = t0; nq1 = t1; nq2 = t2; nq3 = t3;")
            if jflags & JF_POS_NONZERO:
                w("  float vv0, vv1, vv2;")
                g.rot_vec_quat("vv", jpos, nqn)
                w("  np0 = an0 - vv0; np1 = an1 - vv1; np2 = an2 - vv2;")
            w("}")
    # ---- normalise, rotation matrix, range check, save
    if g.pose_fma:
        w("{ const float inv = mjpl::pose_inv_norm(nq0, nq1, nq2, nq3);")
    else:
        w("{ const float inv = __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(nq0 * nq0 + nq1 * nq1 + nq2 * nq2 + nq3 * nq3));")
    w("  q0 = nq0 * inv; q1 = nq1 * inv; q2 = nq2 * inv; q3 = nq3 * inv; }")
    w("p0 = np0; p1 = np1; p2 = np2;")
    w("MJPL_SPEC_QUAT2MAT();")
    w("far = far || !(fmaxf(fabsf(p0), fmaxf(fabsf(p1), fabsf(p2))) <= maxcoord);")
    w("if (far) dead = kInf;")
    if body.save >= 0:
        w(f"{{ float *sv = save + (size_t){body.save} * 7 * sstride;")
        w("  sv[0] = p0; sv[sstride] = p1; sv[2 * sstride] = p2;")
        w("  sv[3 * sstride] = q0; sv[4 * sstride] = q1; sv[5 * sstride] = q2; sv[6 * sstride] = q3; }")


def _emit_geom_pose(g: _Gen, st: _Stage, dp):
    """Centre and z axis of a moving geom (a moving box: its whole frame) from its body's pose."""
    w = g.w
    lpos, lquat = dp[st.geom.doff: st.geom.doff + 3], dp[st.geom.doff + 3: st.geom.doff + 7]
    if st.geom.flags & GF_SAMEPOS:
        w("cx = p0; cy = p1; cz = p2;")
    else:
        for r, nm in enumerate(("cx", "cy", "cz")):
            w(f"{nm} = {_lin3(g, f'p{r}', lpos, r)};")
    if st.geom.flags & GF_SAMEROT:
        w("zx = R2; zy = R5; zz = R8;")
        if st.curbox:
            w("xx = R0; xy = R3; xz = R6; yx = R1; yy = R4; yz = R7;")
    else:
        if g.pose_fma:
            w("{")
            _emit_quat_mul_const(g, "const float", "g", lquat)
        else:
            e = quat_mul_const_right(["q0", "q1", "q2", "q3"], lquat)
            w(f"{{ const float g0 = {e[0]}, g1 = {e[1]}, g2 = {e[2]}, g3 = {e[3]};")
        if st.curbox:  # the whole frame, by the interpreter's own routine (same binary32 values)
            w("  const float gq_[4] = {g0, g1, g2, g3}; float mm_[9]; mjpl::quat2mat(mm_, gq_);")
            w("  zx = mm_[2]; zy = mm_[5]; zz = mm_[8]; xx = mm_[0]; xy = mm_[3]; xz = mm_[6]; yx = mm_[1]; yy = mm_[4]; yz = mm_[7]; }")
        elif g.pose_fma:
            w("  float z_[3]; mjpl::pose_quat2zaxis(z_, g0, g1, g2, g3); zx = z_[0]; zy = z_[1]; zz = z_[2]; }")
        else:
            w("  zx = 2.0f * (g1 * g3 + g0 * g2); zy = 2.0f * (g2 * g3 - g0 * g1); zz = g0 * g0 - g1 * g1 - g2 * g2 + g3 * g3; }")


def _emit_culls(g: _Gen, st: _Stage, prog, fp, cull_form: str, generic: bool, cert_lines):
    """The stage's certificate block (cert_lines; None: a library without the certificate, which carries none of its
    text) and one bounding cull per partner."""
    w = g.w
    cert = cert_lines is not None
    if cert:
        w("deadp = dead;", 2)
        w("if (cert) {", 2)
        for cl in cert_lines:
            w(cl)
        w("}", 2)
    for k, wrow, bound in st.planes:
        ppos = [float(fp[prog.wc_at(wrow, f)]) for f in range(3)]
        at = prog.off_wnarrow + wrow * WN_LEN + WN_ZAXIS
        pz = [float(x) for x in fp[at: at + 3]]
        dot = lin([(pz[0], "cx"), (pz[1], "cy"), (pz[2], "cz")], -(np.float32(pz[0]) * np.float32(ppos[0]) + np.float32(pz[1]) * np.float32(ppos[1]) + np.float32(pz[2]) * np.float32(ppos[2])))
        w(f"MJPL_SPEC_HIT({k}, !({dot} + {'deadp' if cert else 'dead'} > {lit(bound)}));")
    w("const float ux = cx + dead;")
    if cull_form == "expanded" and not generic:
        w(f"const float cc = __builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, ux * ux)){' - wc0' if cert else ''};  // (wc0: the certificate's widening, 0 without)")
    statics = st.statics
    if cull_form == "expanded" and statics:
        for a, b in zip(statics[0::2], statics[1::2]):
            ta, tb = expanded_threshold(a[1:4], a[4], st.reach), expanded_threshold(b[1:4], b[4], st.reach)
            w(f"MJPL_SPEC_CULLX2({a[0]}, {b[0]}, {lit(-2 * a[1])}, {lit(-2 * a[2])}, {lit(-2 * a[3])}, {lit(ta)}, "
              f"{lit(-2 * b[1])}, {lit(-2 * b[2])}, {lit(-2 * b[3])}, {lit(tb)});")
        if len(statics) % 2:
            k, X, Y, Z, bound = statics[-1]
            w(f"MJPL_SPEC_CULLX({k}, {lit(-2 * X)}, {lit(-2 * Y)}, {lit(-2 * Z)}, {lit(expanded_threshold((X, Y, Z), bound, st.reach))});")
    else:
        for a, b in zip(statics[0::2], statics[1::2]):
            w(f"MJPL_SPEC_CULL2({a[0]}, {b[0]}, {lit(a[1])}, {lit(b[1])}, {lit(a[2])}, {lit(b[2])}, {lit(a[3])}, {lit(b[3])}, "
              f"{lit(a[4])}, {lit(b[4])});")
        if len(statics) % 2:
            k, X, Y, Z, bound = statics[-1]
            w(f"MJPL_SPEC_CULL({k}, {lit(X)}, {lit(Y)}, {lit(Z)}, {lit(bound)});")
    for k, n, bound, lvl in st.slots:
        w(f"MJPL_SPEC_SLOTCULL({k}, {n}, {lit(bound)}{f' + ws{lvl}' if cert else ''});")


# the fixed macros of every generated check
_QUAT2MAT = r"""#define MJPL_SPEC_QUAT2MAT() \
  do { float m_[9]; mjpl::pose_quat2mat(m_, q0, q1, q2, q3); R0 = m_[0]; R1 = m_[1]; R2 = m_[2]; R3 = m_[3]; R4 = m_[4]; \
       R5 = m_[5]; R6 = m_[6]; R7 = m_[7]; R8 = m_[8]; } while (0)
"""
_QUAT2MAT_PLAIN = r"""#define MJPL_SPEC_QUAT2MAT() \
  do { R0 = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3; R4 = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3; \
       R8 = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3; R1 = 2.0f * (q1 * q2 - q0 * q3); R2 = 2.0f * (q1 * q3 + q0 * q2); \
       R3 = 2.0f * (q1 * q2 + q0 * q3); R5 = 2.0f * (q2 * q3 - q0 * q1); R6 = 2.0f * (q1 * q3 - q0 * q2); \
       R7 = 2.0f * (q2 * q3 + q0 * q1); } while (0)
"""
_MACROS = r"""typedef float spec_v2f __attribute__((ext_vector_type(2)));
// (a scalar branch around the two v_writelane -- most culls pass for no lane of the wave -- measured
//  3 % SLOWER than parking unconditionally: 213 more branches per configuration)
#define MJPL_SPEC_HIT(k, pass) \
  do { const unsigned long long m_ = __builtin_amdgcn_ballot_w64(pass); \
       mjpl::park_mask<k>(mlo, mhi, m_); } while (0)
// ux = cx, or +inf on a lane that is not to report anything (inactive / decided / out of range)
#define MJPL_SPEC_CULL(k, X, Y, Z, BOUND) \
  do { const float dx_ = ux - (X), dy_ = cy - (Y), dz_ = cz - (Z); \
       MJPL_SPEC_HIT(k, !(mjpl::sqnorm3(dx_, dy_, dz_) > (BOUND))); } while (0)
// two static partners at once: packed float32 arithmetic
#define MJPL_SPEC_CULL2(ka, kb, XA, XB, YA, YB, ZA, ZB, BOUNDA, BOUNDB) \
  do { const spec_v2f dx_ = (spec_v2f){ux, ux} - (spec_v2f){XA, XB}, dy_ = (spec_v2f){cy, cy} - (spec_v2f){YA, YB}, \
                      dz_ = (spec_v2f){cz, cz} - (spec_v2f){ZA, ZB}; \
       const spec_v2f s_ = __builtin_elementwise_fma(dx_, dx_, __builtin_elementwise_fma(dy_, dy_, dz_ * dz_)); \
       const unsigned long long ma_ = __builtin_amdgcn_ballot_w64(!(s_.x > (BOUNDA))); \
       const unsigned long long mb_ = __builtin_amdgcn_ballot_w64(!(s_.y > (BOUNDB))); \
       mjpl::park_mask2<ka, kb>(mlo, mhi, ma_, mb_); } while (0)
// expanded form: t = |c|^2 - 2 c.X against THR = bound - |X|^2 (+ the form's rounding allowance); cc = |c|^2 with
// ux in it, so a lane that is not to report anything carries +inf or NaN here and fails the ordered compare
#define MJPL_SPEC_CULLX(k, M2X, M2Y, M2Z, THR) \
  do { const float t_ = __builtin_fmaf(cz, (M2Z), __builtin_fmaf(cy, (M2Y), __builtin_fmaf(ux, (M2X), cc))); \
       MJPL_SPEC_HIT(k, t_ <= (THR)); } while (0)
#define MJPL_SPEC_CULLX2(ka, kb, AX, AY, AZ, ATHR, BX, BY, BZ, BTHR) \
  do { const float ta_ = __builtin_fmaf(cz, (AZ), __builtin_fmaf(cy, (AY), __builtin_fmaf(ux, (AX), cc))); \
       const float tb_ = __builtin_fmaf(cz, (BZ), __builtin_fmaf(cy, (BY), __builtin_fmaf(ux, (BX), cc))); \
       const unsigned long long ma_ = __builtin_amdgcn_ballot_w64(ta_ <= (ATHR)); \
       const unsigned long long mb_ = __builtin_amdgcn_ballot_w64(tb_ <= (BTHR)); \
       mjpl::park_mask2<ka, kb>(mlo, mhi, ma_, mb_); } while (0)
#define MJPL_SPEC_SLOTCULL(k, n, BOUND) \
  do { const float dx_ = ux - sf.f[0][n], dy_ = cy - sf.f[1][n], dz_ = cz - sf.f[2][n]; \
       MJPL_SPEC_HIT(k, !(mjpl::sqnorm3(dx_, dy_, dz_) > (BOUND))); } while (0)"""


def generate(ip, fp, dp, info, cull_form: str | None = None, generic: bool = False, report: dict | None = None, never_touch=(),
             opts: Options | None = None) -> str:
    """HIP source of `struct Spec` for one compiled program: straight-line filter code.
    generic: the ROBOT's code only -- forward kinematics, geom poses, the culls against earlier moving geoms --
    as literals; every static partner (floor, obstacles, the robot's own world-welded base) is a row of the
    scene table the engine keeps in front of the float32 tables (`tp[-S ...]`, scalar loads): [a0 a1 a2 thr
    desc], tested in one rolled loop per moving geom.  One such library serves the robot in any scene of up
    to 32 static geoms.
    cull_form: "expanded" (default) tests a static partner as  |c|^2 - 2 c.X <= bound - |X|^2  -- three
    fused multiply-adds and a compare per partner on top of one |c|^2 per geom -- with the threshold
    raised by a bound of the form's own rounding (see `expanded_threshold`); "difference" is the
    interpreter's |c - X|^2 <= bound (six operations and a compare, two partners per packed instruction).
    never_touch (dump_never_touch of THIS program -- its hash covers the set): static or plane partners a per-program
    library does not test at all; a scene-generic library tests whatever its scene table holds.
    Moving boxes of one body with one orientation share the slot of their x and y axes; where the program's own slot
    allocation gets in the way of that, every box keeps its own."""
    return _generate(ip, fp, dp, info, cull_form, generic, True, report, never_touch, opts or Options.from_env())


def _generate(ip, fp, dp, info, cull_form: str | None = None, generic: bool = False, share_axes: bool = True, report: dict | None = None,
              never_touch=(), opts: Options = Options()) -> str:
    """generate with the switches as a value; share_axes=False: every moving box keeps its own axes slot from the start."""
    if info.immediate or not info.filter_usable:
        raise ValueError("this model runs the immediate interpreter / has no usable filter: nothing to specialise")
    prog = decode(ip)
    cull_form = cull_form or opts.cull
    skip = set() if generic else {(int(a), int(b)) for a, b in never_touch}
    reach = _body_reach(prog, fp, dp)
    anc, hinges_only = _body_levers(prog, dp)
    levels, nested = _slot_levels(prog, anc, int(info.maxs))
    world = [_world_partners(prog, g, fp, info, generic, skip) for g in prog.geoms]
    statics = [w[1] for w in world]
    axes = (_axes_slots(prog, dp, bool(info.mbox), True, statics) if share_axes else None) or _axes_slots(prog, dp, bool(info.mbox), False, statics)
    stages = [_partners(prog, g, fp, dp, info, generic, world[g.stage], levels[g.stage], axes[g.stage], reach[g.body]) for g in prog.geoms]
    cert = [_certificate(st, dp, anc[st.geom.body]) for st in stages]
    # The certificate is an opt-in build (MJPL_SPEC_CERT=1): measured on the headline batch it halves the waypoint checks and
    # gains 3 % -- a workgroup's two rounds of endpoint tiles bound the launch -- while the lines it adds to the code every
    # tile runs cost 8 % without it (profiles/README.md, round 5).  Without it the generated code carries none of it.
    cert_ok = not generic and hinges_only and nested and all(ok for ok, _, _ in cert) and cull_form == "expanded" and opts.cert
    if report is not None:
        report["cert_ok"], report["cert_levers"] = bool(cert_ok), [levers for _, _, levers in cert]
    # the text of a stage: FK of the bodies since the last stage (trailing bodies without geoms influence nothing: never
    # emitted), the geom's pose, its culls
    text, nbody_done = [], 0
    for st, (_, cert_lines, _) in zip(stages, cert):
        g = _Gen(opts)
        for body in prog.bodies[nbody_done: st.geom.body + 1]:
            g.lines.append("{")
            _emit_body_fk(g, body, dp)
            g.lines.append("}")
        nbody_done = st.geom.body + 1
        _emit_geom_pose(g, st, dp)
        _emit_culls(g, st, prog, fp, cull_form, generic, cert_lines if cert_ok else None)
        text.append(g.lines)
    return _emit_spec(prog, fp, info, stages, text, generic, cert_ok, opts.pose_fma)


def _emit_scene_rows(o):
    """The static partners of a stage of a scene-generic library: the rows of its scene table."""
    o("      {  // static partners: one row [a0 a1 a2 thr] of the scene table each, two rows per scalar load, the next")
    o("         // pair fetched while this one is tested (two buffers taking turns: no copies, 16 scalar registers).")
    o("         // The planes (the last rows): a . c <= thr; the others: |c|^2 + a . c <= thr; a row that is no partner: thr = -inf.")
    o("         // One straight line over all rows, entered at the first pair in use: row offsets and the lanes")
    o("         // the masks are parked in are literals, and what a stage pays beside the tests is the one dispatch (a")
    o("         // rolled loop spent thirty scalar instructions per four rows: addresses, the lane select in M0, the counter).")
    o("        const float ux = cx + dead;")
    o("        const float cc = __builtin_fmaf(cz, cz, __builtin_fmaf(cy, cy, ux * ux));")
    o("        const float zd = 0.0f * ux;  // 0, or NaN on a lane that is not to report anything")
    o("        const float acc_a = sc_nplane >= 2 ? zd : cc, acc_b = sc_nplane >= 1 ? zd : cc;  // (the last two rows)")
    o(f"        FP rows = sc + ({SCENE_HEADER} + g * {SCENE_STAGE});")
    # rows per scalar load: two (two buffers of 8 registers).  Four (2 x 16 registers) measured slower, item pass 0.142 vs
    # 0.137 ms: the kernels sit at the scalar-register limit and spill into vector lanes
    o("        float ra[8], rb[8];")
    o("#define MJPL_SCENE_LOAD(dst, at, n) _Pragma(\"unroll\") for (int k_ = 0; k_ < (n); k_++) dst[k_] = rows[4 * (at) + k_]")
    o("        // (a fetch is waited for behind the arithmetic of the rows before it: scalar loads return out of order, so")
    o("        //  a wait at its first use -- after the NEXT fetch has gone out -- would drain that one, too; `rows` passes")
    o("        //  through the wait so that the next fetch cannot be moved above it, the scheduling barriers keep fetch,")
    o("        //  arithmetic and wait in this order)")
    o("#define MJPL_SCENE_WAIT(buf, n) asm volatile(\"\" : \"+s\"(rows) : \"s\"(buf[0]), \"s\"(buf[(n) - 1]))")
    o("#define MJPL_SCENE_PAIR(buf, acca, accb, ka, kb) do { \\")
    o("          const float t0_ = __builtin_fmaf(cz, (buf)[2], __builtin_fmaf(cy, (buf)[1], __builtin_fmaf(ux, (buf)[0], acca))); \\")
    o("          const float t1_ = __builtin_fmaf(cz, (buf)[6], __builtin_fmaf(cy, (buf)[5], __builtin_fmaf(ux, (buf)[4], accb))); \\")
    o("          const unsigned long long m0_ = __builtin_amdgcn_ballot_w64(t0_ <= (buf)[3]); \\")
    o("          const unsigned long long m1_ = __builtin_amdgcn_ballot_w64(t1_ <= (buf)[7]); \\")
    o("          mjpl::park_mask2<ka, kb>(mlo, mhi, m0_, m1_); } while (0)")
    o("        // (one copy of the line per entry point: falling through case labels, the buffers would arrive at every")
    o("        //  label from two places and the compiler would copy the registers there)")
    o("        switch (sc_first) {")
    for first in range(0, SCENE_ROWS, 2):
        o(f"          {'default' if first == SCENE_ROWS - 2 else f'case {first}'}: {{")
        o(f"        MJPL_SCENE_LOAD(ra, {first}, 8);")
        for k, r in enumerate(range(first, SCENE_ROWS, 2)):  # the rows from `first` on, a pair per fetch
            cur, nxt = ("ra", "rb") if k % 2 == 0 else ("rb", "ra")
            o(f"        MJPL_SCENE_WAIT({cur}, 8);")
            o("        __builtin_amdgcn_sched_barrier(0);")
            if r + 2 < SCENE_ROWS:
                o(f"        MJPL_SCENE_LOAD({nxt}, {r + 2}, 8);")
            o("        __builtin_amdgcn_sched_barrier(0);")
            acc = ("acc_a", "acc_b") if r == SCENE_ROWS - 2 else ("cc", "cc")
            o(f"        MJPL_SCENE_PAIR({cur} + 0, {acc[0]}, {acc[1]}, {r}, {r + 1});")
            o("        __builtin_amdgcn_sched_barrier(0);")
        o("          } break;")
    o("        }")
    o("#undef MJPL_SCENE_LOAD")
    o("#undef MJPL_SCENE_WAIT")
    o("#undef MJPL_SCENE_PAIR")
    o("      }")


def _emit_spec(prog, fp, info, stages, text, generic: bool, cert_ok: bool, pose_fma: bool = False) -> str:
    """The library's float32 check: the fixed macros, the descriptor table, `struct Spec` with the loop around the stages."""
    mbox, maxs, nstage = bool(info.mbox), int(info.maxs), len(stages)
    desc = [st.desc for st in stages]
    out = []
    o = out.append
    o("// GENERATED by mjpl_amd/specialise.py -- straight-line per-configuration check of ONE compiled program.")
    o(f"// program hash {info.hash:016x}, {len(prog.bodies)} moving bodies, {nstage} moving geoms, "
      f"{sum(1 for d in desc for x in d if x)} literal pairs{' (static partners: scene table)' if generic else ''}, slot file width {maxs}")
    o((_QUAT2MAT if pose_fma else _QUAT2MAT_PLAIN) + _MACROS)
    o("")
    o(f"__constant__ int kSpecDesc[{nstage} * 64] = {{")
    for d in desc:
        o("  " + ", ".join(str(x) for x in (d + [0] * (64 - len(d)))) + ",")
    o("};")
    o("")
    if mbox:
        # Whole frames, up to 24 slots: as SlotFile's vectors (<24 x float>, widened to 32 lanes of registers each, six of
        # them) the file alone asks for 192 registers and every access for a contiguous tuple -- 2 KB of scratch per lane
        # at any occupancy.  Every slot number in this code is a literal, so plain scalars serve: the compiler keeps one
        # register per value that is in use (scalar replacement), live from the stage that stores it.
        o(f"struct SpecSlots {{ float f[6][{maxs}]; }};")
        o("static __device__ __forceinline__ void spec_put6(SpecSlots &sf, int slot, const float *t6) {")
        o("#pragma unroll")
        o("  for (int k = 0; k < 6; k++) sf.f[k][slot] = t6[k];")
        o("}")
        o("static __device__ __forceinline__ void spec_get6(const SpecSlots &sf, int slot, float *t6) {")
        o("#pragma unroll")
        o("  for (int k = 0; k < 6; k++) t6[k] = sf.f[k][slot];")
        o("}")
        o("")
    o("struct Spec {")
    o(f"  static constexpr int kNplan = {prog.nplan};")
    o("  // the edge certificate: with ps.adq = this lane's |dq| per planning column, run() widens every bounding cull by what")
    o("  // the pair can move along the edge, every candidate carries that margin to its narrowphase routine, and a lane")
    o("  // none of whose candidates came closer returns V_CLEAR instead of V_NONE (mjpl_fused.h)")
    o(f"  static constexpr bool kCert = {'true' if cert_ok else 'false'};")
    o("  template <class QT>")
    o("  static __device__ __forceinline__ int run(mjpl::FP tp, const float *ltab, const QT *q, int qstride, float *save,")
    o(f"                                            int sstride, bool active, float tol, const mjpl::WaveQueue<float, {'true' if mbox else 'false'}> &wq,")
    o("                                            int item, const mjpl::PatchSink &ps) {")
    o("    using namespace mjpl;")
    o("    SpecSlots sf;" if mbox else f"    SlotFile<float, {maxs}> sf;")
    o("    float p0 = 0, p1 = 0, p2 = 0, q0 = 1, q1 = 0, q2 = 0, q3 = 0;")
    o("    float R0 = 1, R1 = 0, R2 = 0, R3 = 0, R4 = 1, R5 = 0, R6 = 0, R7 = 0, R8 = 1;")
    o("    const int lane = threadIdx.x & 63;")
    o("    const float kInf = __builtin_inff();")
    o("    float dead = active ? 0.0f : kInf;")
    o("    bool far = false;")
    o("    int fl = 0, qn = 0, qb = 0;")
    o("    wq.flags[lane] = (int)((unsigned)item << 3);")
    o("    const _Float16 *adq = kCert ? ps.adq : nullptr;")
    o("    const bool cert = adq != nullptr;  // (wave-uniform)")
    if generic:
        o(f"    // the scene table in front of the float32 tables: header, then per moving geom {SCENE_ROWS} cull rows and {SCENE_ROWS} descriptors")
        o(f"    const FP sc = tp + ({-(SCENE_HEADER + nstage * SCENE_STAGE + 16)});")  # (where the scene table starts, relative to tp)
        o("    const int sc_nplane = info_bits(sc[0]);  // the last 0 .. 2 rows of a geom are planes")
        o("    const int sc_first = info_bits(sc[1]);   // first pair of rows in use (the rows of a geom fill its table from the end)")
        o("    const float maxcoord = sc[4], maxangle = sc[5];")
        o("    const int nwpad = info_bits(sc[2]);")
        o("    const float *lwcull = ltab, *lwnarrow = ltab + info_bits(sc[3]);")
    else:
        o(f"    const float maxcoord = {lit(fp[prog.off_fconst + FC_MAXCOORD])}, maxangle = {lit(fp[prog.off_fconst + FC_MAXANGLE])};")
        o(f"    const int nwpad = {prog.nwpad};")
        o(f"    const float *lwcull = ltab + {prog.off_wcull}, *lwnarrow = ltab + {prog.off_wnarrow};")
    o("#pragma nounroll")
    o(f"    for (int g = 0; g < {nstage}; g++) {{")
    o("      if (__builtin_amdgcn_ballot_w64(dead == 0.0f) == 0ull && qn == 0 && qb == 0) break;  // every lane decided")
    o("      float cx = 0, cy = 0, cz = 0, zx = 0, zy = 0, zz = 0;")
    if mbox:
        o("      float xx = 0, xy = 0, xz = 0, yx = 0, yy = 0, yz = 0;  // a moving box: its x and y axes")
    o("      int mlo = 0, mhi = 0;  // lane k holds the hit mask of this geom's partner k")
    if cert_ok:
        o("      // the certificate's margins of this geom by level (metres; all zero without) and what they widen the culls by")
        o("      float dm0 = 0, dm1 = 0, dm2 = 0, dm3 = 0, dm4 = 0, dm5 = 0, dm6 = 0, dm7 = 0;")
        o("      float wc0 = 0, ws0 = 0, ws1 = 0, ws2 = 0, ws3 = 0, ws4 = 0, ws5 = 0, ws6 = 0, ws7 = 0, deadp = dead;")
    o("      // ... and the descriptor of partner k: one vector load per stage, issued ahead of the stage's")
    o("      // arithmetic (a scalar load per hit stalls the wave for its whole latency)")
    if generic:
        o(f"      const int dv = lane < {SCENE_ROWS} ? info_bits(sc[{SCENE_HEADER} + g * {SCENE_STAGE} + {SCENE_ROWS * 4} + lane]) : kSpecDesc[64 * g + lane];")
    else:
        o("      const int dv = kSpecDesc[64 * g + lane];")
    o("      int gtype = 0, gdoff = 0;")
    o("      switch (g) {")
    for si, (st, lines) in enumerate(zip(stages, text)):
        o(f"        case {si}: {{")
        out.extend("      " + ln for ln in lines)
        o(f"          gtype = {st.geom.type}; gdoff = {f'info_bits(sc[8 + {si}])' if generic else st.geom.doff};")
        o("        } break;")
    o("        default: break;")
    o("      }")
    if generic:
        _emit_scene_rows(o)
    o("      const float cur6[6] = {cx, cy, cz, zx, zy, zz};")
    if mbox:
        o("      const float cur6b[6] = {xx, xy, xz, yx, yy, yz};")
    o("      // partners some lane passed: bit k of the ballot <=> lane k's stored mask is non-zero")
    o("      for (unsigned long long ab = __builtin_amdgcn_ballot_w64((mlo | mhi) != 0); ab; ab &= ab - 1) {")
    o("        const int k = (int)__builtin_ctzll(ab);")
    o("        const unsigned long long pm = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(mlo, k) |")
    o("                                      ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(mhi, k) << 32);")
    o("        const int d = __builtin_amdgcn_readlane(dv, k);")
    o("        const int kind = d & 3, index = (d >> 2) & 255, ptype = (d >> 10) & 15;")
    o("        const bool pfirst = (d >> 14) & 1;")
    o("        // the candidates' certificate margin: this geom's motion relative to the partner (level 0: to the world; 0 without)")
    if cert_ok:
        o("        const int lv_ = (d >> 22) & 7;")
        o("        const float mc_ = lv_ == 0 ? dm0 : (lv_ == 1 ? dm1 : (lv_ == 2 ? dm2 : (lv_ == 3 ? dm3 : (lv_ == 4 ? dm4 : (lv_ == 5 ? dm5 : (lv_ == 6 ? dm6 : dm7))))));")
    else:
        o("        const float mc_ = 0.0f;")
    o("        float t6[6] = {0, 0, 0, 0, 0, 0};")
    if mbox:
        # (a switch over the slots in use keeps every access to the slot file a literal one)
        used1 = sorted({(x >> 2) & 255 for d_ in desc for x in d_ if (x & 3) == EK_SLOT})
        used2 = sorted({(x >> 16) & 63 for d_ in desc for x in d_ if (x & 3) == EK_SLOT} - {63})
        o("        float t6b[6] = {0, 0, 0, 0, 0, 0};")
        o("        const int index2 = (d >> 16) & 63;  // a stored box: the slot of its x and y axes")
        o("        if (kind == EK_SLOT) {")
        for var, used, dst in (("index", used1, "t6"), ("index2", used2, "t6b")):
            o(f"          switch ({var}) {{")
            out.extend(f"            case {n}: spec_get6(sf, {n}, {dst}); break;" for n in used)
            o("            default: break;")
            o("          }")
        o("        }")
    else:
        o("        if (kind == EK_SLOT) slot_get6(sf, index, t6);")
    for cond, box, qv in (("if ((d >> 15) & 1)", "true", "qb"), ("else", "false", "qn")):  # (the box queue's records carry full frames)
        call = f"          queue_push<float, {box}{', true' if mbox else ''}>("
        o("        " + cond)
        o(f"{call}wq, {qv}, dead, fl, active, far, ltab, lwcull, lwnarrow, nwpad, tol, ps, pm, kind, index,")
        o(" " * len(call) + f"gtype, ptype, pfirst, gdoff, cur6, t6, {'cur6b, t6b' if (mbox and box == 'true') else 'nullptr, nullptr'}, mc_);")
    o("      }")
    o("      switch (g) {  // (a literal slot index keeps the slot file in registers)")
    put = "spec_put6" if mbox else "slot_put6"
    for si, st in enumerate(stages):
        if st.geom.store >= 0:
            axes = f" {put}(sf, {st.store2}, cur6b);" if (mbox and st.store2 != 63) else ""
            o(f"        case {si}: {put}(sf, {st.geom.slot}, cur6);{axes} break;")
    o("        default: break;")
    o("      }")
    o("    }")
    m3 = ", true" if mbox else ""
    o(f"    if (qn > 0) queue_drain<float, false, true{m3}>(wq, qn, ltab, lwcull, lwnarrow, nwpad, tol, ps);")
    if mbox or info.wbox or generic:  # (a scene-generic library serves scenes with static boxes whatever scene it was generated from)
        o(f"    if (qb > 0) queue_drain<float, true, true{m3}>(wq, qb, ltab, lwcull, lwnarrow, nwpad, tol, ps);")
    o("    fl = wq.flags[lane] & 7;")
    o("    if (active && far) return V_UNSURE;  // nothing this lane's candidates said can be trusted")
    o("    return !active ? V_NONE : ((fl & 1) ? V_CONTACT : ((fl & 2) ? V_UNSURE : ((cert && !(fl & 4)) ? V_CLEAR : V_NONE)));")
    o("  }")
    o("};")
    return "\n".join(out) + "\n"


def _exact_body_fk(f, body, dp, p, qt, R, sv_prefix: str, sin_tag):
    """mj_kinematics of ONE body op as folded straight-line float64 code (the statements of run_config_queued<double> /
    patch_pairs_body, mjpl_device.h).  (p, qt, R): the walk's current state as Fold values; sv_prefix, sin_tag(joint number):
    how the caller wants a restored pose's values and a hinge's sine and cosine named.  -> new (p, qt, R)."""
    c, v = f.c, f.v
    bd = dp[body.doff:]
    if body.parent == PARENT_CUR:
        pp, pq, pR = p, qt, R
    elif body.parent == PARENT_STATIC:
        pp, pq, pR = [c(x) for x in bd[7:10]], [c(x) for x in bd[10:14]], [c(x) for x in bd[14:23]]
    else:
        k0 = f.n
        f.n += 1
        f.emit(f"const double *sv{k0} = save + (size_t){body.parent - 1} * 7 * sstride;")
        names = [f"{sv_prefix}sv{k0}_{k}" for k in range(7)]
        f.emit("const double " + ", ".join(f"{names[k]} = sv{k0}[{k} * sstride]" for k in range(7)) + ";")
        pp, pq = [v(n) for n in names[:3]], [v(n) for n in names[3:]]
        pR = f.quat2mat(pq)
    np_ = [f.add(x, y) for x, y in zip(f.mul_mat_vec3(pR, [c(x) for x in bd[0:3]]), pp)]
    nq_ = f.mul_quat(pq, [c(x) for x in bd[3:7]])
    for j, (jtype, qsrc, jflags, jdoff) in enumerate(body.joints):
        jd = dp[jdoff:]
        qv = v(f"q[{qsrc} * qstride]") if qsrc >= 0 else c(jd[7])
        dq = f.sub(qv, c(jd[6]))
        jaxis, jpos = [c(x) for x in jd[0:3]], [c(x) for x in jd[3:6]]
        if jtype == JT_SLIDE:
            xaxis = f.rot_vec_quat(jaxis, nq_)
            np_ = [f.add(np_[r], f.mul(xaxis[r], dq)) for r in range(3)]
        else:
            xanchor = np_
            if jflags & JF_POS_NONZERO:
                xanchor = [f.add(x, y) for x, y in zip(f.rot_vec_quat(jpos, nq_), np_)]
            half = f.mul(dq, c(0.5))
            tag = sin_tag(j)
            f.emit(f"double sn{tag}, cs{tag};")
            f.emit(f"sincos_half({f.text(half)}, &sn{tag}, &cs{tag});")
            sn, cs = v(f"sn{tag}"), v(f"cs{tag}")
            nq_ = f.mul_quat(nq_, [cs, f.mul(jaxis[0], sn), f.mul(jaxis[1], sn), f.mul(jaxis[2], sn)])
            if jflags & JF_POS_NONZERO:
                vec = f.rot_vec_quat(jpos, nq_)
                np_ = [f.sub(xanchor[r], vec[r]) for r in range(3)]
    nq_ = f.normalize4(nq_)
    Rn = f.quat2mat(nq_)
    if body.save >= 0:
        f.emit(f"{{ double *sv = save + (size_t){body.save} * 7 * sstride;")
        f.emit("  " + " ".join(f"sv[{k} * sstride] = {f.text(np_[k])};" for k in range(3)))
        f.emit("  " + " ".join(f"sv[{3 + k} * sstride] = {f.text(nq_[k])};" for k in range(4)) + " }")
    return np_, nq_, Rn


def generate_exact(ip, dp, info, generic: bool = False, fold: bool = True) -> str:
    """HIP source of `struct ExactSpec`: the float64 FK of k_patch_pairs (mjpl_filter.h) for one compiled program -- the
    interpreter's own statements, body by body, with the program's constants folded in (mjpl_amd/fold.py: products with
    an exact 0 or 1 and sums with an exact 0 are not executed, the unit-length test of mju_normalize4 is an interval
    test; every other operation in the interpreter's order).  Same values (up to the sign of exact zeros): the kernel's
    verdicts are the interpreter's, bit for bit; what goes away is ~700 scalar loads per wave and more than half of the
    chain's float64 instructions -- the latency of this chain is what a launch's tail kernel costs.
    fold=False: every operation of the statement (tests)."""
    out = []
    o = out.append
    f = Fold(indent="    ", fold=fold)
    c = f.c
    o("struct ExactSpec {")
    o("  // 1: geoms are numbered from the first moving one (a scene-generic library: model ids shift with the scene)")
    o(f"  static constexpr int kRelative = {1 if generic else 0};")
    o("  static __device__ __forceinline__ void fk_pair(const double *q, int qstride, double *save, int sstride, bool active,")
    o("                                                 int ga, int gb, mjpl::GeomT<double> &A, mjpl::GeomT<double> &Bg) {")
    o("    using namespace mjpl;")
    p, qt = [c(0), c(0), c(0)], [c(1), c(0), c(0), c(0)]
    R = [c(x) for x in (1, 0, 0, 0, 1, 0, 0, 0, 1)]
    nsin = itertools.count()  # (the hinges' sines and cosines: numbered through the whole chain)
    for body in decode(ip).bodies:
        f.emit(f"// body op {body.index}")
        p, qt, R = _exact_body_fk(f, body, dp, p, qt, R, "", lambda j: next(nsin))
        for g in body.geoms:
            gd = dp[g.doff:]
            geom_id = g.stage if generic else g.geom_id
            f.emit(f"if (__ballot(active && (ga == {geom_id} || gb == {geom_id})) != 0ull) {{")
            with f.scope():
                ind, f.ind = f.ind, f.ind + "  "
                if g.flags & GF_SAMEPOS:
                    cpos = p
                else:
                    cpos = [f.add(x, y) for x, y in zip(f.mul_mat_vec3(R, [c(x) for x in gd[0:3]]), p)]
                cm = R if g.flags & GF_SAMEROT else f.quat2mat(f.mul_quat(qt, [c(x) for x in gd[3:7]]))
                f.emit(f"const bool isa = ga == {geom_id}, isb = gb == {geom_id};")
                for k in range(3):
                    t = f.text(cpos[k])
                    f.emit(f"A.pos[{k}] = isa ? {t} : A.pos[{k}]; Bg.pos[{k}] = isb ? {t} : Bg.pos[{k}];")
                for k in range(9):
                    t = f.text(cm[k])
                    f.emit(f"A.m[{k}] = isa ? {t} : A.m[{k}]; Bg.m[{k}] = isb ? {t} : Bg.m[{k}];")
                f.ind = ind
            f.emit("}")
    out.extend(f.lines)
    o("  }")
    o("};")
    return "\n".join(out) + "\n"


def generate_full_exact(ip, fp, dp, info, opts: Options | None = None) -> str | None:
    """HIP source of `struct ExactFull`: the float64 check of one configuration through the candidate queues
    (run_config_queued<double>, mjpl_device.h -- what k_edges_fused_f64 calls for every endpoint and waypoint when the
    filter is off or refused) as straight-line code for ONE compiled program: forward kinematics and geom poses with the
    constants folded in (mjpl_amd/fold.py), one bounding cull per ENABLED partner with its row of the table as literals,
    the interpreter's own pushes, drains and narrowphase routines behind them.  The culls are the interpreter's
    expressions (|c - X|^2 as x x + y y + z z, + dead, against the same bound), so the same candidates reach the same
    routines: the verdicts are the interpreter's bit for bit.  None: the model keeps the interpreting kernel (moving
    boxes, a slot file wider than 16, the immediate interpreter).
    MEASURED (round 5, tools/f64_probe.py): no faster than the interpreting kernel -- 0.4497 against 0.4473 ms per 262 144
    edges.  The interpreter fetches four partners' rows with one sixteen-value scalar load; every float64 literal here
    is two scalar moves, and the kernel spills 222 scalar registers.  So libraries carry it only when built with
    MJPL_SPEC_F64=1; what a generated float64 path would need is the partners' rows from the table (scalar loads) around
    the folded FK -- the FK is a tenth of the check."""
    opts = opts or Options.from_env()
    if info.immediate or info.mbox or int(info.maxs) > 16:
        return None
    prog = decode(ip)
    nwpad, maxs, off_wcull, off_wnarrow = prog.nwpad, int(info.maxs), prog.off_wcull, prog.off_wnarrow
    state = ["p0", "p1", "p2", "q0", "q1", "q2", "q3"] + [f"R{k}" for k in range(9)]
    stages, desc, pending = [], [], []
    for body in prog.bodies:
        b = body.index
        f = Fold(indent="          ", prefix=f"b{b}_")
        if b == 0:  # the walk's state is still a generation-time constant (nothing assigned to the variables yet)
            p, qt, R = [f.c(0)] * 3, [f.c(1), f.c(0), f.c(0), f.c(0)], [f.c(x) for x in (1, 0, 0, 0, 1, 0, 0, 0, 1)]
        else:
            p, qt, R = [f.v(n) for n in state[:3]], [f.v(n) for n in state[3:7]], [f.v(n) for n in state[7:]]
        p, qt, R = _exact_body_fk(f, body, dp, p, qt, R, f.prefix, lambda j: f"b{b}j{j}")
        for name, val in zip(state, p + qt + R):
            f.emit(f"{name} = {f.text(val)};")
        pending.extend(["        {"] + f.lines + ["        }"])
        for gm in body.geoms:
            gd = dp[gm.doff:]
            g = Fold(indent="          ", prefix=f"g{len(stages)}_")
            sp_, sq_, sR_ = [g.v(n) for n in state[:3]], [g.v(n) for n in state[3:7]], [g.v(n) for n in state[7:]]
            cpos = sp_ if gm.flags & GF_SAMEPOS else [g.add(x, y) for x, y in zip(g.mul_mat_vec3(sR_, [g.c(x) for x in gd[0:3]]), sp_)]
            if gm.flags & GF_SAMEROT:
                zax = [sR_[2], sR_[5], sR_[8]]
            else:  # quat2zaxis(qt (x) lq): the third column of quat2mat, its expressions
                gq = g.mul_quat(sq_, [g.c(x) for x in gd[3:7]])
                m_ = g.mul
                q00, q01, q02 = m_(gq[0], gq[0]), m_(gq[0], gq[1]), m_(gq[0], gq[2])
                q11, q13, q22, q23, q33 = m_(gq[1], gq[1]), m_(gq[1], gq[3]), m_(gq[2], gq[2]), m_(gq[2], gq[3]), m_(gq[3], gq[3])
                two = g.c(2.0)
                zax = [m_(two, g.add(q13, q02)), m_(two, g.sub(q23, q01)), g.add(g.sub(g.sub(q00, q11), q22), q33)]
            for name, val in zip(("cx", "cy", "cz", "zx", "zy", "zz"), cpos + zax):
                g.emit(f"{name} = {g.text(val)};")
            cv = [g.v("cx"), g.v("cy"), g.v("cz")]
            partners = []
            wbound = gd[GD_WBOUND: GD_WBOUND + nwpad]
            sbound = gd[GD_WBOUND + 2 * nwpad: GD_WBOUND + 2 * nwpad + MAX_SLOTS]
            for wrow in gm.world_rows(planes=True):
                ppos = [g.c(dp[prog.wc_at(wrow, k)]) for k in range(3)]
                pz = [g.c(dp[off_wnarrow + wrow * WN_LEN + WN_ZAXIS + k]) for k in range(3)]
                dif = [g.sub(cv[k], ppos[k]) for k in range(3)]
                dot = g.sum([g.mul(dif[k], pz[k]) for k in range(3)])
                g.emit(f"MJPL_X64_HIT({len(partners)}, !({g.text(dot)} + dead > {dlit(wbound[wrow])}));")
                partners.append(pack_desc(EK_PLANE, wrow, GT_PLANE, 1, 0))
            for wrow in gm.world_rows(planes=False):  # other static geoms
                ptype, pgid = prog.row_info(dp, wrow)
                pfirst = 1 if (ptype < gm.type or (ptype == gm.type and pgid < gm.geom_id)) else 0
                dd = [g.sub(cv[k], g.c(dp[prog.wc_at(wrow, k)])) for k in range(3)]
                sq = g.sum([g.mul(x, x) for x in dd])
                g.emit(f"MJPL_X64_HIT({len(partners)}, !({g.text(sq)} + dead > {dlit(wbound[wrow])}));")
                partners.append(pack_desc(EK_STATIC, wrow, ptype, pfirst, 1 if ptype == GT_BOX else 0))
            for n, pw in gm.slots(maxs):  # earlier moving geoms in the slot file
                g.emit(f"MJPL_X64_SLOTCULL({len(partners)}, {n}, {dlit(sbound[n])});")
                partners.append(pack_desc(EK_SLOT, n, (pw >> 12) & 15, 1 if (pw & P_FIRST) else 0, 0))
            if len(partners) > 64:
                return None
            stages.append((pending + g.lines, gm.type, gm.doff, gm.slot))
            pending = []
            desc.append(partners)
    nstage = len(stages)
    wbox = any((x >> 15) & 1 for d in desc for x in d)
    out = []
    o = out.append
    o(f"// GENERATED: the float64 check of program {info.hash:016x} through the candidate queues -- {nstage} moving geoms, "
      f"{sum(len(d) for d in desc)} literal pairs")
    o("#define MJPL_X64_HIT(k, pass) \\")
    o("  do { const unsigned long long m_ = __builtin_amdgcn_ballot_w64(pass); \\")
    o("       mjpl::park_mask<k>(mlo, mhi, m_); } while (0)")
    o("#define MJPL_X64_SLOTCULL(k, n, BOUND) \\")
    o("  do { const double dx_ = cx - sf.f[0][n], dy_ = cy - sf.f[1][n], dz_ = cz - sf.f[2][n]; \\")
    o("       MJPL_X64_HIT(k, !(dx_ * dx_ + dy_ * dy_ + dz_ * dz_ + dead > (BOUND))); } while (0)")
    o(f"__constant__ int kExactDesc[{nstage} * 64] = {{")
    for d in desc:
        o("  " + ", ".join(str(x) for x in (d + [0] * (64 - len(d)))) + ",")
    o("};")
    o("struct ExactFull {")
    o(f"  static constexpr int kMaxs = {maxs};")
    # (outlined: inlined at the pool kernel's one call site the build returned no contact for any waypoint tile while endpoint
    #  tiles were right -- every variant with a second call site, and this outlined form, return the interpreter's verdicts on
    #  all edges; observed with ROCm 7.2's compiler at 222 spilled scalar registers, not explained)
    # (MJPL_SPEC_F64_INLINE=1: the inlined form, for tools/f64_inline_probe.py -- the experiment that looks for what breaks it)
    attr = "always_inline" if opts.f64_inline else "noinline"
    o(f"  static __device__ __attribute__(({attr})) int run(const double *ltab, const double *q, int qstride, double *save, int sstride, bool active,")
    o("                                            const mjpl::WaveQueue<double, false> &wq, int item, const mjpl::PatchSink &ps) {")
    o("    using namespace mjpl;")
    o(f"    SlotFile<double, {maxs}> sf;")
    o("    double p0 = 0, p1 = 0, p2 = 0, q0 = 1, q1 = 0, q2 = 0, q3 = 0;")
    o("    double R0 = 1, R1 = 0, R2 = 0, R3 = 0, R4 = 1, R5 = 0, R6 = 0, R7 = 0, R8 = 1;")
    o("    const int lane = threadIdx.x & 63;")
    o("    double dead = active ? 0.0 : (double)__builtin_inff();")
    o("    int fl = 0, qn = 0, qb = 0;")
    o("    wq.flags[lane] = (int)((unsigned)item << 3);")
    o(f"    const int nwpad = {nwpad};")
    o(f"    const double *lwcull = ltab + {off_wcull}, *lwnarrow = ltab + {off_wnarrow};")
    o("#pragma nounroll")
    o(f"    for (int g = 0; g < {nstage}; g++) {{")
    o("      if (__builtin_amdgcn_ballot_w64(dead == 0.0) == 0ull && qn == 0 && qb == 0) break;  // every lane decided")
    o("      double cx = 0, cy = 0, cz = 0, zx = 0, zy = 0, zz = 0;")
    o("      int mlo = 0, mhi = 0;  // lane k holds the hit mask of this geom's partner k")
    o("      const int dv = kExactDesc[64 * g + lane];")
    o("      int gtype = 0, gdoff = 0;")
    o("      switch (g) {")
    for si, (lines, gtype, gdoff, store) in enumerate(stages):
        o(f"        case {si}: {{")
        out.extend(lines)
        o(f"          gtype = {gtype}; gdoff = {gdoff};")
        o("        } break;")
    o("        default: break;")
    o("      }")
    o("      const double cur6[6] = {cx, cy, cz, zx, zy, zz};")
    o("      for (unsigned long long ab = __builtin_amdgcn_ballot_w64((mlo | mhi) != 0); ab; ab &= ab - 1) {")
    o("        const int k = (int)__builtin_ctzll(ab);")
    o("        const unsigned long long pm = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(mlo, k) |")
    o("                                      ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(mhi, k) << 32);")
    o("        const int d = __builtin_amdgcn_readlane(dv, k);")
    o("        const int kind = d & 3, index = (d >> 2) & 255, ptype = (d >> 10) & 15;")
    o("        const bool pfirst = (d >> 14) & 1;")
    o("        double t6[6] = {0, 0, 0, 0, 0, 0};")
    o("        if (kind == EK_SLOT) slot_get6(sf, index, t6);")
    o("        if ((d >> 15) & 1)")
    o("          queue_push<double, true>(wq, qb, dead, fl, active, false, ltab, lwcull, lwnarrow, nwpad, 0.0, ps, pm, kind, index, gtype, ptype,")
    o("                                   pfirst, gdoff, cur6, t6);")
    o("        else")
    o("          queue_push<double, false>(wq, qn, dead, fl, active, false, ltab, lwcull, lwnarrow, nwpad, 0.0, ps, pm, kind, index, gtype, ptype,")
    o("                                    pfirst, gdoff, cur6, t6);")
    o("      }")
    o("      switch (g) {  // (a literal slot index keeps the slot file in registers)")
    for si, (_, _, _, store) in enumerate(stages):
        if store >= 0:
            o(f"        case {si}: slot_put6(sf, {store}, cur6); break;")
    o("        default: break;")
    o("      }")
    o("    }")
    o("    if (qn > 0) queue_drain<double, false, true>(wq, qn, ltab, lwcull, lwnarrow, nwpad, 0.0, ps);")
    if wbox:
        o("    if (qb > 0) queue_drain<double, true, true>(wq, qb, ltab, lwcull, lwnarrow, nwpad, 0.0, ps);")
    o("    fl = wq.flags[lane] & 3;")
    o("    return !active ? V_NONE : ((fl & 1) ? V_CONTACT : V_NONE);")
    o("  }")
    o("};")
    return "\n".join(out) + "\n"


_TU = """// GENERATED translation unit: the float32 filter kernels of mjpl_filter.h around one model's Spec.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
%(waves_define)s%(pose_include)s#include "mjpl_filter.h"
#include "mjpl_project.h"

namespace {
%(spec)s
%(exact)s
%(exact_full)s
}  // namespace

using namespace mjpl;
#define SPEC_GRANT(kern)                                                                            \\
  static std::atomic<size_t> granted{0};  /* (engines of several threads share the library) */      \\
  if (lds > granted.load(std::memory_order_relaxed)) {                                              \\
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1; \\
    size_t have = granted.load(std::memory_order_relaxed);                                          \\
    while (have < lds && !granted.compare_exchange_weak(have, lds, std::memory_order_relaxed)) {}   \\
  }
#define SPEC_LAUNCH(kern, ...)                                                                      \\
  do {                                                                                              \\
    SPEC_GRANT(kern)                                                                                \\
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, __VA_ARGS__);                        \\
    return hipGetLastError() == hipSuccess ? 0 : -1;                                                \\
  } while (0)

extern "C" {
int mjpl_spec_abi(void) { return MJPL_SPEC_ABI; }
unsigned long long mjpl_spec_src_stamp(void) { return MJPL_SRC_STAMP; }
// 0: the whole program in literals; else rows per moving geom << 8 | moving geoms of a scene-generic library
int mjpl_spec_generic(void) { return %(generic)d; }
unsigned long long mjpl_spec_hash(void) { return 0x%(hash)016xull; }
int mjpl_spec_launch_configs(hipStream_t st, unsigned grid, unsigned block, size_t lds, const int *ip, int nip, const float *fp,
                             int nfp, const double *Q, int64_t N, int layout, float tol, uint8_t *valid, int *ulist, int *ucount,
                             UndecidedConfigs uc, int *zero_next) {
  SPEC_LAUNCH((k_filter_configs<Spec, %(maxs)d, %(wbox)s, %(mbox)s>), ip, nip, fp, nfp, Q, N, layout, tol, valid, ulist, ucount, uc,
              zero_next);
}
int mjpl_spec_launch_endpoints(hipStream_t st, unsigned grid, unsigned block, size_t lds, const int *ip, int nip, const float *fp,
                               int nfp, const double *QA, const double *QB, int64_t E, int layout, float tol, uint8_t *valid,
                               int32_t *first_bad, int *status, int *ulist, int *ucount, UndecidedConfigs uc, int *slist,
                               int *scount, ItemBuffers ib, double step, int *zero_next) {
  SPEC_LAUNCH((k_filter_endpoints<Spec, %(maxs)d, %(wbox)s, %(mbox)s>), ip, nip, fp, nfp, QA, QB, E, layout, tol, valid, first_bad, status,
              ulist, ucount, uc, slist, scount, ib, step, zero_next);
}
int mjpl_spec_launch_items(hipStream_t st, unsigned grid, unsigned block, size_t lds, const int *ip, int nip, const float *fp,
                           int nfp, ItemBuffers ib, EdgeSource src, float tol, uint8_t *valid, int32_t *first_bad, int *ulist, int *ucount,
                           UndecidedConfigs uc) {
  SPEC_LAUNCH((k_filter_items<Spec, %(maxs)d, %(wbox)s, %(mbox)s>), ip, nip, fp, nfp, ib, src, tol, valid, first_bad, ulist, ucount, uc);
}
// persistent kernels (one wave per tile of 64, tiles from a device counter): the launcher sizes the grid
int mjpl_spec_launch_endpoints_pw(hipStream_t st, size_t lds, const int *ip, int nip, const float *fp, int nfp, const double *QA,
                                  const double *QB, int64_t E, int layout, float tol, uint8_t *valid, int32_t *first_bad,
                                  int *status, int *ulist, int *ucount, UndecidedConfigs uc, ItemBuffers ib, double step,
                                  int *zero_next, int *tiles) {
  auto kern = k_filter_endpoints_pw<Spec, %(maxs)d, %(wbox)s, %(mbox)s>;
  SPEC_GRANT(kern);
  const unsigned grid = persistent_grid(kern, lds, (E + 63) / 64);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, ip, nip, fp, nfp, QA, QB, E, layout, tol, valid, first_bad, status, ulist,
                     ucount, uc, ib, step, zero_next, tiles);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int mjpl_spec_launch_items_pw(hipStream_t st, size_t lds, const int *ip, int nip, const float *fp, int nfp, ItemBuffers ib,
                              EdgeSource src, float tol, uint8_t *valid, int32_t *first_bad, int *ulist, int *ucount,
                              UndecidedConfigs uc, int *tiles) {
  auto kern = k_filter_items_pw<Spec, %(maxs)d, %(wbox)s, %(mbox)s>;
  SPEC_GRANT(kern);
  const unsigned grid = persistent_grid(kern, lds, (long long)ib.cap / 64);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kBlock), lds, st, ip, nip, fp, nfp, ib, src, tol, valid, first_bad, ulist, ucount, uc, tiles);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int mjpl_spec_launch_tail(hipStream_t st, size_t lds, TailArgs a) {
  auto kern = k_tail<ExactSpec, %(maxs)d, %(maxsd)d, %(wbox)s, %(mbox)s>;
  SPEC_GRANT(kern);
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.nw + a.np + a.nx)), dim3(kBlock), lds, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// the whole float32 filter of an edge launch as one kernel (mjpl_fused.h); nwaves: wavefronts per workgroup, which
// must be what mjpl_spec_fused_waves reports (twelve at three waves per SIMD; eight for a model with moving boxes,
// whose code is built for two)
int mjpl_spec_fused_waves(void) { return %(fwaves)d; }
// 1: the library's check was generated with the edge certificate (MJPL_SPEC_CERT=1): its fused kernel keeps |QB - QA| rows in LDS
int mjpl_spec_fused_cert(void) { return Spec::kCert ? 1 : 0; }
int mjpl_spec_launch_fused(hipStream_t st, int nwaves, size_t lds, FusedArgs a) {
  if (nwaves != %(fwaves)d) return -1;
  auto kern = k_edges_fused<Spec, %(maxs)d, %(wbox)s, %(mbox)s, %(fwaves)d>;
  SPEC_GRANT(kern);
  return fused_launch(kern, nwaves, lds, a, st) == hipSuccess ? 0 : -1;
}
%(fused_f64)s
int mjpl_spec_launch_patch(hipStream_t st, unsigned grid, unsigned block, size_t lds, const int *ip, int nip, const double *dp,
                           int ndp, GeomTable gt, UndecidedConfigs uc, uint8_t *valid, int32_t *first_bad) {
  SPEC_LAUNCH((k_patch_pairs<ExactSpec>), ip, nip, dp, ndp, gt, uc, valid, first_bad);
}
}
// ---- PoseConstraint projections of this model's site bodies (mjpl_project.h)
%(pose)s
"""


# ---- the PoseConstraint projection as straight-line code (mjpl_project.h: PoseStatic<PS>) ----------------------
PH_NBODY, PH_NJOINT, PH_NQ, PH_SIZE = 0, 1, 2, 6  # (mjpl_pose.h)


def dump_pose_chain(model, site_body: int):
    """The chain program mjpl_pose_chain_dump compiles for (model, site body), on the host (no GPU)
    -> (pi int32[], pd float64[], hash)."""
    lib = _engine.load_library()
    d, keep = _engine._model_desc(model)
    npi, npd, h = C.c_int32(0), C.c_int32(0), C.c_uint64(0)

    def args(bufs):
        pi, pd = bufs or (None, None)
        return [C.byref(d), int(site_body), _ptr(pi, _engine._I32P), C.byref(npi), _ptr(pd, _engine._F64P), C.byref(npd), C.byref(h)]
    pi, pd = _engine._sized_call(lib, lib.mjpl_pose_chain_dump, args, lambda _: (np.zeros(npi.value, np.int32), np.zeros(npd.value, np.float64)))
    return pi, pd, int(h.value)


def pose_site_bodies(model) -> list[int]:
    """The bodies a generated projection is made for: every body that carries a site (a PoseConstraint names a site)."""
    return sorted({int(b) for b in np.asarray(model.site_bodyid).reshape(-1) if int(b) > 0})


def generate_pose(pi, pd, hash_: int, index: int, qualifier: str = "static __device__ __forceinline__", fold: bool = True) -> str:
    """`struct PoseSpec<index>`: mj_kinematics along one chain with the model's constants folded in (mjpl_amd/fold.py):
    the operations of pose_chain (mjpl_pose.h) in the same order, minus those whose result the constants decide
    (products with an exact 0 or 1, sums with an exact 0) -- the same float64 values up to the sign of exact zeros.
    The half-angle sines and cosines of the hinges are arguments: the caller computes them, one joint after the other
    or one joint per lane of a row's group (mjpl_project.h).  What goes away against the interpreting kernel: the
    reading of the chain program, the loop control, the trip through LDS of the joints' axes and anchors, and about
    half of the chain's arithmetic.  qualifier: how the member functions are declared (tests compile a chain for the host)."""
    nb, nj, nq = int(pi[PH_NBODY]), int(pi[PH_NJOINT]), int(pi[PH_NQ])
    f = Fold(indent="    ", fold=fold)  # (fold=False: every operation of the statement, for tests)
    c, v = f.c, f.v
    jtypes, qadrs, jids, q0s = [], [], [], []
    p, qt = [c(0), c(0), c(0)], [c(1), c(0), c(0), c(0)]
    R = [c(x) for x in (1, 0, 0, 0, 1, 0, 0, 0, 1)]
    ic, dc, jk = PH_SIZE, 0, 0
    for b in range(nb):
        njnt = int(pi[ic]); ic += 1
        f.emit(f"// chain body {b}")
        bpos, bquat = [c(x) for x in pd[dc:dc + 3]], [c(x) for x in pd[dc + 3:dc + 7]]
        dc += 7
        np_ = [f.add(x, y) for x, y in zip(f.mul_mat_vec3(R, bpos), p)]
        nq_ = f.mul_quat(qt, bquat)
        for j in range(njnt):
            jtype, qadr, jid = int(pi[ic]), int(pi[ic + 1]), int(pi[ic + 2]); ic += 3
            jtypes.append(jtype); qadrs.append(qadr); jids.append(jid); q0s.append(float(pd[dc + 6]))
            jaxis, jpos = [c(x) for x in pd[dc:dc + 3]], [c(x) for x in pd[dc + 3:dc + 6]]
            dq = f.sub(v(f"q[{qadr}]"), c(pd[dc + 6]))
            dc += 7
            xaxis = f.rot_vec_quat(jaxis, nq_)
            xanchor = [f.add(x, y) for x, y in zip(f.rot_vec_quat(jpos, nq_), np_)]
            for r in range(3):
                f.emit(f"jx[{jk}][{r}] = {f.text(xaxis[r])}; jx[{jk}][{3 + r}] = {f.text(xanchor[r])};")
            if jtype == JT_SLIDE:
                np_ = [f.add(np_[r], f.mul(xaxis[r], dq)) for r in range(3)]
            else:
                sn, cs = v(f"sn[{jk}]"), v(f"cs[{jk}]")
                qloc = [cs, f.mul(jaxis[0], sn), f.mul(jaxis[1], sn), f.mul(jaxis[2], sn)]
                nq_ = f.mul_quat(nq_, qloc)
                vec = f.rot_vec_quat(jpos, nq_)
                np_ = [f.sub(xanchor[r], vec[r]) for r in range(3)]
            jk += 1
        nq_ = f.normalize4(nq_)
        p, qt = np_, nq_
        R = f.quat2mat(qt)
    assert jk == nj
    f.emit("// the site (mj_local2Global)")
    spos = [v(f"tail[mjpl::PT_SITE_POS + {k}]") for k in range(3)]
    squat = [v(f"tail[mjpl::PT_SITE_QUAT + {k}]") for k in range(4)]
    sp = f.mul_mat_vec3(R, spos)
    for k in range(3):
        f.emit(f"out.site_xpos[{k}] = {f.text(f.add(sp[k], p[k]))};")
    sm = f.quat2mat(f.mul_quat(qt, squat))
    for k in range(9):
        f.emit(f"out.site_xmat[{k}] = {f.text(sm[k])};")
    out = []
    o = out.append
    njx = max(nj, 1)
    tab = lambda vals: ", ".join(str(x) for x in vals) or "0"  # noqa: E731
    o(f"// GENERATED: chain program {hash_:016x} -- {nb} bodies, {nj} joints, nq {nq}; "
      f"{f.ops['mul']} products, {f.ops['add']} sums, {f.ops['sqrt']} square roots after folding")
    o(f"struct PoseSpec{index} {{")
    o(f"  static constexpr int kNQ = {nq}, kNJ = {nj};")
    o(f"  static constexpr unsigned long long kHash = 0x{hash_:016x}ull;")
    o(f"  {qualifier} constexpr int jtype(int k) {{ constexpr int t[{njx}] = {{{tab(jtypes)}}}; return t[k]; }}")
    o(f"  {qualifier} constexpr int qadr(int k) {{ constexpr int t[{njx}] = {{{tab(qadrs)}}}; return t[k]; }}")
    o(f"  {qualifier} constexpr int jid(int k) {{ constexpr int t[{njx}] = {{{tab(jids)}}}; return t[k]; }}")
    o("  // half the angle of chain joint k (a hinge's: what its sine and cosine are taken of; 0 for a slide joint)")
    o(f"  {qualifier} double half_angle(int k, const double (&q)[{nq}]) {{")
    o("    switch (k) {")
    for k in range(nj):
        if jtypes[k] == JT_HINGE:
            h = Fold(indent="")
            o(f"      case {k}: return {h.text(h.sub(h.v(f'q[{qadrs[k]}]'), h.c(q0s[k])))} * 0.5;" if q0s[k] == 0.0 else
              f"      case {k}: return (q[{qadrs[k]}] - {dlit(q0s[k])}) * 0.5;")
    o("      default: return 0.0;")
    o("    }")
    o("  }")
    o(f"  {qualifier} void chain(const double (&q)[{nq}], const double (&sn)[{njx}], const double (&cs)[{njx}], double (&jx)[{njx}][6],")
    o("                                               mjpl::PoseChainOut &out, const double *tail) {")
    out.extend(f.lines)
    o("  }")
    o("};")
    return "\n".join(out) + "\n"


def generate_pose_section(model, nplan: int = 0, qidx=None) -> str:
    """All generated projections of a model and the entry points a library exports for them.  nplan: the number of
    planning joints of the program the library is built for (the planner's chunk kernel keeps a lane's rows in
    registers when it is a constant; 0: unknown); qidx: their qpos addresses (None: unknown -- the kernels read the
    planner's table)."""
    specs = []
    for k, b in enumerate(pose_site_bodies(model)):
        pi, pd, h = dump_pose_chain(model, b)
        if int(pi[PH_NJOINT]) == 0 or int(pi[PH_NJOINT]) > 12 or int(pi[PH_NQ]) > 16:
            continue  # (nothing to project / registers: the interpreting kernels serve such a chain)
        specs.append((len(specs), h, generate_pose(pi, pd, h, len(specs))))
    n = len(specs)
    np_ = int(nplan) if 0 < int(nplan) <= 16 else 0
    planq = "mjpl::PlanQRuntime"
    plan_src = []
    if np_ and qidx is not None and len(qidx) == np_:
        planq = "SpecPlanQ"
        plan_src = ["// where the program's planning columns sit in qpos (the library is named by the program's hash, which covers them)",
                    "struct SpecPlanQ {",
                    "  static __device__ __forceinline__ constexpr int at(int k, const int *) {",
                    f"    constexpr int t[{np_}] = {{{', '.join(str(int(x)) for x in qidx)}}};",
                    "    return t[k];", "  }", "};"]
    src = ["namespace {"] + [s for _, _, s in specs] + plan_src + ["}  // namespace", "", 'extern "C" {', f"int mjpl_spec_pose_count(void) {{ return {n}; }}",
           "unsigned long long mjpl_spec_pose_hash(int k) {", "  switch (k) {"]
    src += [f"    case {k}: return PoseSpec{k}::kHash;" for k, _, _ in specs]
    src += ["    default: return 0ull;", "  }", "}"]
    # Launchers of the row kernels (mjpl_rows.h).  G: lanes per row (1, 4 or 8); return 0 = launched, -1 = refused with
    # nothing launched (no such projection / lane count / number of planning joints: the caller takes the interpreting
    # kernel), -2 = the launch failed (a HIP error the caller reports; hipGetLastError has cleared it).
    done = ["    default: return -1;", "  }", "  return hipGetLastError() == hipSuccess ? 0 : -2;", "}"]

    def cases(fmt):
        out = []
        for k, _, _ in specs:
            out += [f"    case {3 * k + i}: " + fmt.format(k=k, g=g) + " break;" for i, g in enumerate((1, 4, 8))]
        return out
    pick = ["  if (G != 1 && G != 4 && G != 8) return -1;", "  switch (3 * k + (G == 8 ? 2 : (G == 4 ? 1 : 0))) {"]
    src += ["int mjpl_spec_launch_pose_apply(int k, int G, hipStream_t st, unsigned grid, const int *pi, const double *pd, const double *Qold,",
            "                                const double *Q, int64_t N, int64_t per, double *Qout, uint8_t *ok, int32_t *iters, mjpl::PosePhase ph) {"] + pick
    src += cases("hipLaunchKernelGGL((mjpl::k_pose_apply_rows<PoseSpec{k}, {g}>), dim3(grid), dim3(mjpl::kPoseBlock), 0, st, pi, pd, Qold, Q, N, per, Qout, ok, iters, ph);")
    src += done
    src += ["int mjpl_spec_launch_gen_project(int k, int G, hipStream_t st, unsigned grid, int L, int nplan, int S, double eps, int par, const int *pi,",
            "                                 const double *pd, const int *qidx, const double *qbase, const uint8_t *isplan, const double *lo,",
            "                                 const double *hi, const double *Tgt, mjpl::RrtLanes ln, mjpl::RrtCand cd, int *ctr) {"]
    if np_:
        src += [f"  if (nplan != {np_}) return -1;  // (the library's program plans {np_} joints)",
                "  if (G == 16 || G == 64) {  // sixteen lanes per row, four rows per wave or one: the next step's first Newton pass beside this step's closing evaluation (mjpl_rows.h)",
                "    switch (2 * k + (G == 64 ? 1 : 0)) {"]
        src += [f"      case {2 * k + i}: hipLaunchKernelGGL((mjpl::k_rrt_gen_project_ahead<PoseSpec{k}, {np_}, {rows}, {planq}>), dim3(grid), dim3(mjpl::kPoseBlock), 0, st, L, S, eps, par, pi, pd, qidx, qbase, isplan, lo, hi, Tgt, ln, cd, ctr); break;"
                for k, _, _ in specs for i, rows in enumerate((4, 1))]
        src += ["      default: return -1;", "    }", "    return hipGetLastError() == hipSuccess ? 0 : -2;", "  }"] + pick
        src += cases("hipLaunchKernelGGL((mjpl::k_rrt_gen_project_rows<PoseSpec{k}, " + str(np_) + ", {g}, " + planq + ">), dim3(grid), dim3(mjpl::kPoseBlock), 0, st, L, S, eps, par, pi, pd, qidx, qbase, isplan, lo, hi, Tgt, ln, cd, ctr);")
        src += done
    else:
        src += ["  return -1;  // (the number of planning joints is not a constant of this library)", "}"]
    src += ["int mjpl_spec_launch_ik_solve(int k, int G, hipStream_t st, unsigned grid, const int *pi, const double *pd, const double *Q, int64_t N, int64_t per,",
            "                               double *Qout, uint8_t *ok, int32_t *iters, double *err, int max_restarts, unsigned long long restart_seed) {"] + pick
    src += cases("hipLaunchKernelGGL((mjpl::k_ik_solve_rows<PoseSpec{k}, {g}>), dim3(grid), dim3(mjpl::kPoseBlock), 0, st, pi, pd, Q, N, per, Qout, ok, iters, err, max_restarts, (uint64_t)restart_seed);")
    src += done + ["}"]
    return "\n".join(src) + "\n"


_FUSED_F64 = """// the float64 checks of an edge launch through the pool (filter off or refused) around this model's generated check
int mjpl_spec_launch_fused_f64(hipStream_t st, int nwaves, size_t lds, FusedArgs a) {
  if (nwaves != kFusedF64Waves) return -1;
  auto kern = k_edges_fused_f64<ExactFull::kMaxs, %(wbox)s, false, kFusedF64Waves, true, ExactFull>;
  SPEC_GRANT(kern);
  return fused_launch(kern, nwaves, lds, a, st) == hipSuccess ? 0 : -2;
}"""


_POSE_INCLUDE = '#include "mjpl_pose_f32.h"\n'  # (a unit whose generated check calls the fused helpers)


def translation_unit(spec: str, exact: str, key: int, info, generic_word: int = 0, pose: str | None = None, exact_full: str | None = None,
                     opts: Options | None = None) -> str:
    """The source of a library: the kernels of mjpl_filter.h / mjpl_fused.h instantiated around `spec` / `exact`,
    and the projections of `pose` (generate_pose_section; None: a library without any)."""
    opts = opts or Options.from_env()
    mbox = bool(info.mbox)
    if pose is None:
        pose = 'extern "C" int mjpl_spec_pose_count(void) { return 0; }\n'
    wbox_s = "true" if (info.wbox or generic_word or mbox) else "false"
    return _TU % dict(spec=spec, exact=exact, hash=key, maxs=info.maxs, pose=pose, exact_full=exact_full or "",
                      fused_f64=(_FUSED_F64 % dict(wbox=wbox_s)) if exact_full else "", wbox=wbox_s, mbox="true" if mbox else "false",
                      maxsd=32 if mbox else info.maxs,  # (the exact kernels of a model with moving boxes: the general build)
                      # a model with moving boxes keeps whole frames in its slot file and in the box queue's records: built for
                      # two waves per SIMD (256 VGPRs), eight waves per workgroup of the fused kernel -- at three the kernels
                      # spill 60 .. 90 registers and the fused kernel's LDS no longer fits: 0.56 against 0.42 ms on Franka-P
                      # with the ten pad boxes (profiles/r04_pads.json)
                      fwaves=(4 * opts.mbox_waves) if mbox else 12,
                      waves_define=f"#define MJPL_SPEC_WAVES {opts.mbox_waves}\n" if mbox else "",
                      pose_include=_POSE_INCLUDE if (opts.pose_fma or opts.sincos) else "",
                      generic=generic_word)


def spec_path(hash_: int, generic: bool = False) -> str:
    return os.path.join(SPEC_DIR, f"libmjpl_spec{'g' if generic else ''}_{hash_:016x}.so")


# every Python file the generated text depends on: a library older than one of them is stale
GENERATOR_SOURCES = tuple(os.path.join(os.path.dirname(os.path.abspath(__file__)), f) for f in ("specialise.py", "program.py", "fold.py"))


def library_source(model, allowed_collision_bodies=(), qidx=None, qpos_base=None, filter_tol: float = 0.0, generic: bool = False,
                   prune_contacts: int = 1, opts: Options | None = None) -> tuple | None:
    """The source half of build(): (the hash the library is named by, its translation unit), or None if the model cannot
    be specialised.  Host Python over the program tables: no compiler, no GPU."""
    opts = opts or Options.from_env()
    ip, fp, dp, info = dump_program(model, allowed_collision_bodies, qidx, qpos_base, filter_tol)
    if info.immediate or not info.filter_usable or (generic and not info.scene_ok):
        return None
    never_touch, _, never_hash, _ = dump_never_touch(model, allowed_collision_bodies, qidx, qpos_base, filter_tol, prune_contacts=prune_contacts)
    if prune_contacts == 1 and never_hash != int(info.hash):
        raise RuntimeError("dump_never_touch and dump_program disagree on the program hash")
    info.hash = never_hash
    key = info.robot_hash if generic else info.hash
    prog = decode(ip)
    src = translation_unit(generate(ip, fp, dp, info, generic=generic, never_touch=never_touch, opts=opts), generate_exact(ip, dp, info, generic=generic),
                           key, info, (SCENE_ROWS << 8 | prog.nstage) if generic else 0,  # (kSceneRows, moving geoms)
                           pose=generate_pose_section(model, prog.nplan, qidx=(None if qidx is None else [int(x) for x in qidx])),
                           # (an experiment, off by default: see generate_full_exact / mjpl_fused.h)
                           exact_full=generate_full_exact(ip, fp, dp, info, opts) if (not generic and opts.f64) else None, opts=opts)
    return key, src


def build(model, allowed_collision_bodies=(), qidx=None, qpos_base=None, filter_tol: float = 0.0, force: bool = False,
          keep_source: bool = True, extra_flags=(), output: str | None = None, generic: bool = False, prune_contacts: int = 1,
          overlay: bool = True, uniform_regions: bool = True, opts: Options | None = None) -> str | None:
    """Generate and compile the specialised library of (model, planning set, tolerance).  Returns the
    path of the library, or None if the model cannot be specialised (immediate interpreter).
    generic: the ROBOT's scene-generic library instead (named by the robot hash): built from any scene that
    holds the robot, it serves every scene with it -- the static geoms come from the engine's scene table.
    prune_contacts: the engine option of that name the library is for (0: the program without its never-touch set, which
    an engine with the option off looks for -- A/B measurements).
    overlay: False leaves mjpl_overlay.h (build.overlay_flags) off the compiler's line: the same text, the same hash, the
    same values from the plain templates of mjpl_device.h -- the comparison build of tests/test_gpu_overlay.py.
    uniform_regions: False leaves build.codegen_flags' option off the line in the same way: the compiler's default control
    flow, the same values -- the comparison build of tests/test_gpu_uniform_regions.py.
    opts: the generation switches (None: Options.for_build() -- the environment's, the fused pose arithmetic on).
    Options.for_build()._replace(pose_fma=False, sincos=False) writes the pose arithmetic as plain expressions and calls
    sincosf: the same program hash, so give such a library an `output` outside SPEC_DIR's top level, where no engine looks
    on its own -- the comparison build of tests/test_gpu_pose_fma.py."""
    made = library_source(model, allowed_collision_bodies, qidx, qpos_base, filter_tol, generic, prune_contacts, opts or Options.for_build())
    if made is None:
        return None
    key, src = made
    os.makedirs(SPEC_DIR, exist_ok=True)
    target = output or spec_path(key, generic)  # (output, extra_flags: timing-only variants, tools/time_variants.sh)
    deps = [os.path.join(_build.CSRC, f) for f in _build.STAMPED_HEADERS] + [_build.OVERLAY_HEADER, _build.POSE_HEADER] + list(GENERATOR_SOURCES)
    if not force and os.path.exists(target) and all(os.path.getmtime(d) <= os.path.getmtime(target) for d in deps):
        return target
    return _compile(src, os.path.join(SPEC_DIR, f"spec{'g' if generic else ''}_{key:016x}.hip"), target, keep_source, extra_flags, overlay, uniform_regions)


def _compile(src: str, src_path: str, target: str, keep_source: bool, extra_flags, overlay: bool = True, uniform_regions: bool = True) -> str:
    """The compile half of build(): `src` through hipcc into `target`; with keep_source the text stays as `src_path`."""
    # Source and library appear under their final names complete or not at all (os.replace): an engine created
    # while a rebuild is running finds the old library or the new one, never half a file -- a failed dlopen would
    # be remembered as "no library" for the life of that process -- and two builds of one hash cannot interleave.
    tag = f".tmp{os.getpid()}_{threading.get_ident():x}"
    src_tmp = src_path[:-4] + tag + ".hip"
    lib_tmp = target + tag
    with open(src_tmp, "w") as f:
        f.write(src)
    # -fno-slp-vectorize: left alone, the SLP vectoriser pairs the scalar binary32 arithmetic of the generated
    # code into v_pk_* instructions -- which issue no faster than the two instructions they replace -- at the
    # price of ~700 v_mov to assemble the pairs and of spilled registers: 0.279 -> 0.259 ms per step
    cmd = [_build.hipcc(), *_build.hipcc_flags(), "-fno-slp-vectorize", "-Wno-unused-variable", "-Wno-unused-but-set-variable", f"-I{_build.CSRC}",
           *(_build.overlay_flags() if overlay else ()), *_build.codegen_flags(uniform_regions), *extra_flags, "-o", lib_tmp, src_tmp]
    try:
        subprocess.run(cmd, check=True)
        os.replace(lib_tmp, target)
        if keep_source:
            os.replace(src_tmp, src_path)
    finally:
        for leftover in (lib_tmp, src_tmp):
            if os.path.exists(leftover):
                os.remove(leftover)
    return target


def _main(argv=None) -> int:
    """python -m mjpl_amd.specialise MODEL.xml [--joints a,b,...] [--keyframe NAME] [--allowed bodyA:bodyB,...]
    Builds the specialised library for (model, planning joints, base configuration) -- a deployment step:
    needs hipcc, no GPU; engines created for that combination afterwards load it by program hash."""
    import argparse

    from .model import load_mjcf
    ap = argparse.ArgumentParser(prog="python -m mjpl_amd.specialise", description=_main.__doc__)
    ap.add_argument("mjcf", help="primitive-only MJCF file")
    ap.add_argument("--joints", default="", help="comma-separated planning joints (default: all)")
    ap.add_argument("--keyframe", default="", help="keyframe holding the non-planning joints (default: qpos0)")
    ap.add_argument("--allowed", default="", help="allowed collision body pairs, bodyA:bodyB,...")
    ap.add_argument("--tol", type=float, default=0.0, help="filter tolerance in metres (0: the model's default)")
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--generic", action="store_true",
                    help="the robot's scene-generic library: static geoms (<= 32) come from a table, so obstacles may change "
                         "without a compiler (about 10 % slower than the scene's own library)")
    args = ap.parse_args(argv)
    model = load_mjcf(args.mjcf)
    names = [n for n in args.joints.split(",") if n]
    qidx = None
    if names:
        qidx = np.asarray([int(model.jnt_qposadr[model.joint(n).id]) for n in names], dtype=np.int32)
    base = model.keyframe(args.keyframe).qpos.copy() if args.keyframe else None
    allowed = tuple(tuple(p.split(":")) for p in args.allowed.split(",") if p)
    path = build(model, allowed, qidx, base, args.tol, force=args.force, generic=args.generic)
    print(path if path else "this model runs the general builds: nothing to specialise")
    return 0


if __name__ == "__main__":
    raise SystemExit(_main())
