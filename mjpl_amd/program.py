"""The layout of a compiled program's control words `ip` (mjpl_device.h) and its one decoder: what the generators of
mjpl_amd/specialise.py walk is the plain data `decode` returns, never the words themselves."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

H_NBODYOPS, H_NPLAN, H_NSAVE, H_NSLOTS, H_OFF_BODYOPS, H_OFF_PERM, H_OFF_WCULL, H_OFF_WNARROW, H_NWORLD, H_NWPAD, \
    H_OFF_FCONST, H_SIZE = range(12)
B_PARENT, B_DOFF, B_BODYID, B_NJNT, B_SAVE, B_NGEOM, B_SIZE = range(7)
J_TYPE, J_QSRC, J_FLAGS, J_DOFF, J_SIZE = range(5)
G_TYPE, G_FLAGS, G_DOFF, G_STORE, G_GEOMID, G_SMASK, G_WMASK_LO, G_WMASK_HI, G_PMASK_LO, G_PMASK_HI, G_SIZE = range(11)
MAX_SLOTS = 32
GD_SIZE, GD_WBOUND = 7, 12
GF_SAMEPOS, GF_SAMEROT = 1, 2
JF_POS_NONZERO = 1
PARENT_CUR, PARENT_STATIC = 0, -1
JT_SLIDE, JT_HINGE = 2, 3
GT_PLANE, GT_SPHERE, GT_CAPSULE, GT_BOX = 0, 2, 3, 6
EK_PLANE, EK_STATIC, EK_SLOT = 0, 1, 2
WN_ZAXIS, WN_LEN = 0, 12
P_FIRST = 1 << 17
SLOT_NONE = 63
FC_MAXCOORD, FC_MAXANGLE = 0, 1


class Joint(NamedTuple):
    type: int
    qsrc: int     # planning column, or < 0: held at its constant
    flags: int
    doff: int     # its constants in dp: axis, anchor, qpos0, the constant


class Geom(NamedTuple):
    stage: int    # number among the moving geoms
    body: int     # index of its body op
    type: int
    flags: int
    doff: int
    store: int    # < 0: not stored; else slot | slot of a box's x and y axes << 6
    geom_id: int
    smask: int
    wmask: int    # static partners by world row (64 bits), pmask: the planes among them
    pmask: int
    swords: tuple  # the 32 slot words: what each slot holds for this geom

    @property
    def slot(self) -> int:
        return self.store & 63 if self.store >= 0 else -1

    def slots(self, maxs: int = MAX_SLOTS) -> list:
        """[(slot, its word)] of the earlier moving geoms this one is tested against."""
        return [(n, self.swords[n]) for n in range(maxs) if (self.smask >> n) & 1]

    def world_rows(self, planes: bool) -> list:
        mask = self.pmask if planes else self.wmask
        return [r for r in range(64) if (mask >> r) & 1]


class Body(NamedTuple):
    index: int
    parent: int   # PARENT_CUR, PARENT_STATIC, or 1 + the save slot of its parent's pose
    doff: int
    save: int     # slot its own pose is saved in, or < 0
    joints: tuple
    geoms: tuple


class Program(NamedTuple):
    nplan: int
    nwpad: int
    off_wcull: int
    off_wnarrow: int
    off_fconst: int
    bodies: tuple

    @property
    def geoms(self) -> list:
        return [g for b in self.bodies for g in b.geoms]

    @property
    def nstage(self) -> int:
        return sum(len(b.geoms) for b in self.bodies)

    def wc_at(self, wrow: int, f: int) -> int:
        """Where field f (x, y, z, info) of world row `wrow` sits in the float tables: rows in chunks of four, field-major."""
        return self.off_wcull + ((wrow >> 2) << 4) + (f << 2) + (wrow & 3)

    def row_info(self, tab, wrow: int) -> tuple:
        """(geom type, geom id) of a world row: the integer its info field carries in the low 32 bits (tab: fp or dp)."""
        at = self.wc_at(wrow, 3)
        word = int(np.frombuffer(tab[at:at + 1].tobytes()[:4], dtype=np.int32)[0])
        return word & 255, word >> 8


def decode(ip) -> Program:
    """The control words of a compiled program as plain data: body ops in order, each with its joints and moving geoms."""
    def u64(lo, hi):
        return (int(lo) & 0xFFFFFFFF) | ((int(hi) & 0xFFFFFFFF) << 32)
    bodies, stage, pc = [], 0, int(ip[H_OFF_BODYOPS])
    for b in range(int(ip[H_NBODYOPS])):
        parent, bdoff, njnt, save, ngeom = (int(ip[pc + k]) for k in (B_PARENT, B_DOFF, B_NJNT, B_SAVE, B_NGEOM))
        pc += B_SIZE
        joints = tuple(Joint(*(int(ip[pc + j * J_SIZE + k]) for k in (J_TYPE, J_QSRC, J_FLAGS, J_DOFF))) for j in range(njnt))
        pc += njnt * J_SIZE
        geoms = []
        for _ in range(ngeom):
            w = [int(x) for x in ip[pc: pc + G_SIZE + MAX_SLOTS]]
            geoms.append(Geom(stage, b, w[G_TYPE], w[G_FLAGS], w[G_DOFF], w[G_STORE], w[G_GEOMID], w[G_SMASK],
                              u64(w[G_WMASK_LO], w[G_WMASK_HI]), u64(w[G_PMASK_LO], w[G_PMASK_HI]), tuple(w[G_SIZE:])))
            stage += 1
            pc += G_SIZE + MAX_SLOTS
        bodies.append(Body(b, parent, bdoff, save, joints, tuple(geoms)))
    return Program(int(ip[H_NPLAN]), int(ip[H_NWPAD]), int(ip[H_OFF_WCULL]), int(ip[H_OFF_WNARROW]), int(ip[H_OFF_FCONST]), tuple(bodies))
