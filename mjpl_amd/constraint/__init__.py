"""Constraint plug-in surface of the MI355X build: the ABC, the four concrete constraints and
the two composition helpers (obeys / apply).  Collision and pose validation run in
``libmjpl_hip.so``, as does the push of the clearance constraint; joint limits are a NumPy box test."""
from . import certified_intervals as _cert
from . import clearance_constraint as _cl
from . import collision_constraint as _cc
from . import constraint_interface as _ci
from . import joint_limit_constraint as _jl
from . import pose_constraint as _pc
from . import utils as _u

Constraint = _ci.Constraint
CollisionConstraint, CollisionRuleset = _cc.CollisionConstraint, _cc.CollisionRuleset
ClearanceConstraint = _cl.ClearanceConstraint
CertifiedIntervals = _cert.CertifiedIntervals
JointLimitConstraint = _jl.JointLimitConstraint
PoseConstraint = _pc.PoseConstraint
obeys_constraints, apply_constraints = _u.obeys_constraints, _u.apply_constraints

__all__ = ["Constraint", "CertifiedIntervals", "ClearanceConstraint", "CollisionConstraint", "CollisionRuleset", "JointLimitConstraint", "PoseConstraint",
           "obeys_constraints", "apply_constraints"]
