"""Independent NumPy float64 statement of the clearance gradient (include/mjpl_hip.h: mjpl_clearance_grad*).

* Joint frames: world axis and anchor of every joint, as forward kinematics moves it.  A body's frame starts
  from its parent's pose (the CPU oracle's forward kinematics, oracle.pyoracle: fk) and the body offset, and
  its joints are applied one after the other: a joint's axis and anchor are taken in the frame its earlier
  joints left (MuJoCo's xaxis / xanchor).
* Point Jacobian: J(x in body b)[:, j] = axis_j x (x - anchor_j) for a hinge, axis_j for a slide, for the
  joints of b and of its ancestors; 0 for every other joint.
* Clearance gradient: n . (J2(w2) - J1(w1)) from witness points and a normal.
* Signed point-to-geom distances (sphere, capsule, box, plane), to tell whether a point lies on a surface.

Nothing of the product's kernels is used.
"""
import numpy as np

import distance_reference as ref

HINGE, SLIDE = 3, 2


def _qmul(a, b):
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0)
    w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def _qrot(q, v):
    """rotate v [..., 3] by the unit quaternions q [..., 4]"""
    u = q[..., 1:]
    t = 2 * np.cross(u, v)
    return v + q[..., :1] * t + np.cross(u, t)


def joint_frames(model, Q, fk):
    """World axis and anchor of every joint at the full-nq configurations Q [N, nq] -> ([N, njnt, 3], [N, njnt, 3]).
    fk: the oracle's forward kinematics of Q (parent poses)."""
    Q = np.asarray(Q, float)
    n = Q.shape[0]
    axes, anchors = np.zeros((n, model.njnt, 3)), np.zeros((n, model.njnt, 3))
    for b in range(1, model.nbody):
        nj = int(model.body_jntnum[b])
        if nj == 0:
            continue
        p = int(model.body_parentid[b])
        pq = fk["xquat"][:, p]
        pos = fk["xpos"][:, p] + _qrot(pq, np.broadcast_to(model.body_pos[b], (n, 3)))
        quat = _qmul(pq, np.broadcast_to(model.body_quat[b], (n, 4)))
        for j in range(int(model.body_jntadr[b]), int(model.body_jntadr[b]) + nj):
            a = np.asarray(model.jnt_axis[j], float)
            jp = np.asarray(model.jnt_pos[j], float)
            qa = int(model.jnt_qposadr[j])
            dq = Q[:, qa] - model.qpos0[qa]
            xaxis = _qrot(quat, np.broadcast_to(a, (n, 3)))
            xanchor = pos + _qrot(quat, np.broadcast_to(jp, (n, 3)))
            axes[:, j], anchors[:, j] = xaxis, xanchor
            if model.jnt_type[j] == SLIDE:
                pos = pos + xaxis * dq[:, None]
            else:
                loc = np.concatenate([np.cos(dq / 2)[:, None], np.sin(dq / 2)[:, None] * a], axis=1)
                quat = _qmul(quat, loc)
                quat = quat / np.linalg.norm(quat, axis=1, keepdims=True)
                pos = xanchor - _qrot(quat, np.broadcast_to(jp, (n, 3)))
    return axes, anchors


def moved_by(model):
    """bool [nbody, njnt]: joint j moves body b (j's body is b or one of its ancestors)"""
    out = np.zeros((model.nbody, model.njnt), bool)
    jb = np.asarray(model.jnt_bodyid)
    for b in range(model.nbody):
        a = b
        while True:
            out[b] |= jb == a
            if a == 0:
                break
            a = int(model.body_parentid[a])
    return out


def point_jacobian(model, axes, anchors, bodies, x, cols=None):
    """J [N, 3, ncols] of the world points x [N, 3] fixed to bodies [N] (int), over the qpos columns `cols`
    (default: every joint, nq == njnt here)."""
    x = np.asarray(x, float)
    n = x.shape[0]
    cols = np.arange(model.nq) if cols is None else np.asarray(cols)
    jnt_of = np.empty(model.nq, int)
    jnt_of[np.asarray(model.jnt_qposadr)] = np.arange(model.njnt)
    J = np.zeros((n, 3, len(cols)))
    mv = moved_by(model)
    for c, qa in enumerate(cols):
        j = jnt_of[qa]
        v = axes[:, j] if model.jnt_type[j] == SLIDE else np.cross(axes[:, j], x - anchors[:, j])
        J[:, :, c] = v * mv[np.asarray(bodies), j][:, None]
    return J


def clearance_gradient(model, Q, pair_geoms, fromto, normal, cols=None, fk=None):
    """n . (J2(w2) - J1(w1)) [N, ncols]: pair_geoms [N, 2] (g1, g2), fromto [N, 6], normal [N, 3]."""
    from oracle import pyoracle
    fk = pyoracle.Oracle(model).fk(np.asarray(Q, float)) if fk is None else fk
    axes, anchors = joint_frames(model, Q, fk)
    gb = np.asarray(model.geom_bodyid)
    J1 = point_jacobian(model, axes, anchors, gb[pair_geoms[:, 0]], fromto[:, :3], cols)
    J2 = point_jacobian(model, axes, anchors, gb[pair_geoms[:, 1]], fromto[:, 3:], cols)
    return np.einsum("ni,nij->nj", normal, J2 - J1)


def point_geom_distance(t, pos, mat, size, x):
    """Signed distance of the points x [N, 3] to geoms of type t with poses pos [N, 3], mat [N, 9], size [N, 3]
    (negative inside; a plane is the half-space below its z axis)."""
    pos, mat, size, x = (np.asarray(a, float) for a in (pos, mat, size, x))
    if t == ref.PLANE:
        return ref._dot(x - pos, mat[..., [2, 5, 8]])
    if t == ref.SPHERE:
        return ref._norm(x - pos) - size[..., 0]
    if t == ref.CAPSULE:
        a, b = ref._core(t, pos, mat, size)
        return ref.pt_seg(x, a, b) - size[..., 0]
    if t == ref.BOX:
        return ref.point_box(x, pos, mat, size)
    raise ValueError(f"geom type {t}")
