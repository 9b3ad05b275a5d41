#!/usr/bin/env python3
"""A trajectory with a certificate for its whole curve: the wall case of DESIGN.md 5.13 on the MI355X.

    python examples/certified_trajectory.py

A ball (r 0.01) on a slide and a wall 2 mm thick at x = 0.9.  The path [0, 0.8, 0.81, 0] stays 0.079 clear of the wall on
every straight segment, but the spline through it -- what a trajectory follows -- peaks at 0.926, past the wall.  The
straight-segment certificate says FREE, the spline certificate says HIT and where, and generate_certified_trajectory adds
the waypoints that keep the curve clear.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mjpl_amd as mjpl  # noqa: E402
from mjpl_amd import engine  # noqa: E402

STATUS = {engine.SWEEP_FREE: "FREE", engine.SWEEP_HIT: "HIT", engine.SWEEP_UNDECIDED: "UNDECIDED",
          engine.SWEEP_NONFINITE: "NONFINITE", engine.SWEEP_RANGE: "RANGE"}


def main() -> bool:
    mb = mjpl.ModelBuilder()
    mb.add_body("ball", pos=(0, 0, 1))
    mb.add_joint("ball", "ball_slide_x", "slide", axis=(1, 0, 0), range=(-2, 2))
    mb.add_geom("ball", "sphere", (0.01,))
    mb.add_geom("world", "box", (0.001, 0.5, 0.5), pos=(0.9, 0, 1), name="wall")
    cc = mjpl.CollisionConstraint(mb.compile())
    sweep = dict(cap=0.1, lo=[-2.0], hi=[2.0])

    path = [np.array([x]) for x in (0.0, 0.8, 0.81, 0.0)]
    segments = [STATUS[cc.certified_interval(a, b, **sweep).status] for a, b in zip(path[:-1], path[1:])]
    print(f"straight segments: {segments}")
    cert = cc.certified_spline(path, **sweep)
    print(f"spline: {STATUS[cert.status]} in piece {cert.piece} at s = {cert.s_hit:.4f}, x = {cert.q_hit[0]:.4f}")

    generator = mjpl.HipToppTrajectoryGenerator(0.01, [1.0], [2.0], engine=cc.engine)
    out = mjpl.generate_certified_trajectory(path, generator, [cc], cc, **sweep)
    if out is None:
        print("no certified trajectory")
        return False
    traj, cert = out
    print(f"certified: {STATUS[cert.status]} over {len(cert.piece_status)} pieces, clearance >= {cert.clear_lb:.4f} all along; "
          f"{len(traj.positions)} states, largest x {max(float(q[0]) for q in traj.positions):.4f}")
    return True


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
