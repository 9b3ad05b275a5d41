/*
 * mjpl_hip.h -- C ABI of libmjpl_hip.so, the MI355X (gfx950) batched collision-validation
 * engine that sits behind mjpl's Constraint plug-in surface.
 *
 * The reference (adlarkin/mjpl, pure Python) has no FFI for this path: its
 * CollisionConstraint calls the third-party MuJoCo engine through pybind, one
 * configuration at a time.  Each entry point below names the reference interface
 * (file:line under /root/reference) whose work it replaces; INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions: plain pointers and sizes, caller owns every buffer, every function returns
 * an int status (MJPL_OK = 0) and never throws; mjpl_last_error() returns a thread-local
 * message for the last non-zero status.  One engine per thread/stream.  There is NO CPU
 * fallback: without a gfx950 device mjpl_create fails with MJPL_E_NODEVICE.
 *
 * Batch layout: a batch holds only the nplan PLANNING columns of qpos (the joints a
 * planner samples, rrt.py:162-206); the remaining qpos entries come from the template
 * given to mjpl_set_planning.  layout = MJPL_SOA: Q[c*N + i] (coalesced column reads,
 * the native layout); layout = MJPL_AOS: Q[i*nplan + c] (numpy row-major, transposed
 * through LDS inside the kernel).
 */
#ifndef MJPL_HIP_H
#define MJPL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MJPL_OK            0
#define MJPL_E_ARG        -1   /* bad argument (NULL, negative size, step_dist <= 0 ...)      */
#define MJPL_E_JOINT      -2   /* joint type outside {slide, hinge} (reference README.md:20)  */
#define MJPL_E_PAIRTYPE   -3   /* a colliding geom pair has no primitive narrowphase routine  */
#define MJPL_E_CAPACITY   -4   /* model exceeds a compiled-in limit (slots, LDS)              */
#define MJPL_E_NODEVICE   -5   /* no usable HIP device                                        */
#define MJPL_E_HIP        -6   /* HIP runtime error (message in mjpl_last_error)              */
#define MJPL_E_NONFINITE  -7   /* NaN/inf edge (the reference's waypoint loop would not end)  */

#define MJPL_SOA 0
#define MJPL_AOS 1

/* mjpl_check_edges flags */
#define MJPL_EDGE_INTERIOR_ONLY 1  /* skip check 0 (the endpoint): exactly _valid_collision_interval */

/* mjtJoint / mjtGeom values */
#define MJPL_JNT_SLIDE 2
#define MJPL_JNT_HINGE 3
#define MJPL_GEOM_PLANE 0
#define MJPL_GEOM_SPHERE 2
#define MJPL_GEOM_CAPSULE 3
#define MJPL_GEOM_BOX 6

/* The mjModel subset the path reads; field names as in mjModel.  Replaces the
 * `model: mujoco.MjModel` argument of CollisionConstraint.__init__
 * (src/mjpl/constraint/collision_constraint.py:10-24).  Arrays are borrowed for the
 * duration of mjpl_create only. */
typedef struct mjpl_model_desc {
  int32_t nq, njnt, nbody, ngeom;
  const int32_t *body_parentid;    /* [nbody]   */
  const int32_t *body_weldid;      /* [nbody]   */
  const int32_t *body_jntadr;      /* [nbody]   */
  const int32_t *body_jntnum;      /* [nbody]   */
  const double  *body_pos;         /* [nbody*3] */
  const double  *body_quat;        /* [nbody*4] */
  const int32_t *jnt_type;         /* [njnt]    */
  const int32_t *jnt_qposadr;      /* [njnt]    */
  const double  *jnt_axis;         /* [njnt*3]  */
  const double  *jnt_pos;          /* [njnt*3]  */
  const double  *qpos0;            /* [nq]      */
  const int32_t *geom_type;        /* [ngeom]   */
  const int32_t *geom_bodyid;      /* [ngeom]   */
  const int32_t *geom_contype;     /* [ngeom]   */
  const int32_t *geom_conaffinity; /* [ngeom]   */
  const double  *geom_size;        /* [ngeom*3] */
  const double  *geom_pos;         /* [ngeom*3] */
  const double  *geom_quat;        /* [ngeom*4] */
  const double  *geom_rbound;      /* [ngeom]   */
  const double  *geom_margin;      /* [ngeom]   */
} mjpl_model_desc;

typedef struct mjpl_engine mjpl_engine;

typedef struct mjpl_info {
  int32_t device;            /* HIP device ordinal                                   */
  int32_t nplan;             /* planning columns per configuration                    */
  int32_t nmoving_geoms;     /* geoms on bodies below a joint                         */
  int32_t nstatic_geoms;     /* geoms welded to the world (poses folded at create)    */
  int32_t npairs;            /* geom pairs left after the mj_collision filters + a6   */
  int32_t npairs_world;      /* ... of which moving-vs-static                         */
  int32_t nslots;            /* register slots holding earlier moving geoms           */
  int32_t nsaves;            /* LDS pose saves for branching bodies                   */
  int32_t lds_bytes_configs; /* dynamic LDS per block, configs kernel                 */
  int32_t lds_bytes_edges;   /* dynamic LDS per block, edges kernel                   */
  int32_t block_threads;
  int32_t compute_units;
  int32_t filter_enabled;    /* float32 filter in front of the exact kernels              */
  float   filter_tol;        /* its tolerance band, metres                                */
  int32_t lds_bytes_filter;  /* dynamic LDS per block, float32 filter kernels             */
  int32_t filter_block_threads;
  char    arch[32];          /* gcnArchName, e.g. "gfx950:sramecc+:xnack-"            */
  /* the filter's binary32 error bound for this model: a float32 signed distance is
   * within filter_err_a + filter_err_b * C of the float64 one while every moving coordinate
   * magnitude is <= C; configurations beyond filter_max_coord go to the float64 kernels */
  float   filter_max_coord;
  float   filter_err_a;
  float   filter_err_b;
  int32_t filter_poisoned_geoms; /* static geoms too large / far for binary32: always re-checked */
  /* which float32 interpreter this model runs: 0 = queued narrowphase, small builds (no moving
   * boxes, <= 16 stored geoms); 1 = queued, the general 24-slot build with moving boxes in the
   * box queue; 2 = immediate narrowphase (more than 24 stored geoms, or MJPL_FORCE_IMMEDIATE=1
   * at creation: tests).  A specialised library can replace 0 and 1 (mjpl_spec_loaded), not 2. */
  int32_t filter_interpreter;
  /* how an edge launch is laid out on the device (defaults; MJPL_PERSIST / MJPL_TAIL at creation):
   * persistent_kernels = 1: endpoint and item kernels run as persistent grids of waves with tile queues;
   * fused_tail = 1: walking kernel, pair re-check and exact edge kernel are roles of one launch (k_tail) */
  int32_t persistent_kernels;
  int32_t fused_tail;
  /* fused_edges = 1 (default where the model runs the queued float32 interpreter or its own kernels; MJPL_FUSED=0
   * at creation restores the two persistent kernels): ONE filter kernel per edge launch -- endpoint tiles and
   * waypoint tiles of a batch served by the same resident workgroups from a work pool in LDS (k_edges_fused) --
   * followed by k_tail.  With the filter off (filter_enabled = 0) the float64 checks take the same route
   * (k_edges_fused_f64, then k_check_edges over the edges too long for the pool).  fused_waves: wavefronts per
   * workgroup of that kernel. */
  int32_t fused_edges;
  int32_t fused_waves;
} mjpl_info;

/* ---- lifetime ------------------------------------------------------------------ */

/* CollisionConstraint.__init__ + CollisionRuleset.__init__
 * (collision_constraint.py:10-24, :42-64).  allowed_bodies: nallowed body-id pairs
 * (any order inside a pair).  The mj_collision pair filters (contype/conaffinity,
 * same weld body, weld parent-child) and the allowed-body-pair ruleset
 * (collision_constraint.py:66-95) are folded into a static pair list here. */
int mjpl_create(const mjpl_model_desc *model, const int32_t *allowed_bodies, int32_t nallowed,
                int32_t device, mjpl_engine **out);
void mjpl_destroy(mjpl_engine *e);

/* Which qpos entries a batch column feeds, and the template for all others
 * (planners keep non-planning joints at q_init, rrt.py:205-206; :162-172).
 * Default after create: nplan = nq, qidx = 0..nq-1, template = qpos0. */
int mjpl_set_planning(mjpl_engine *e, const int32_t *qidx, int32_t nplan, const double *qpos_base);

int mjpl_get_info(const mjpl_engine *e, mjpl_info *out);

/* Verdicts are always those of the exact float64 kernels.  By default a float32 FILTER kernel
 * runs first: the same algorithms in binary32, every comparison against a contact threshold
 * classified with a tolerance `tol` (metres) as certain / uncertain; only the items it cannot
 * decide are re-run by the float64 kernel (same stream, no host round trip).  enable = 0
 * sends everything through the float64 kernels.  Environment overrides at create:
 * MJPL_FILTER=0|1, MJPL_FILTER_TOL=<metres>.
 * Half of `tol` is the budget for the binary32 rounding error of this model's poses, which
 * mjpl_create bounds from the kinematic chain (mjpl_info.filter_err_a / _b).  The default tolerance
 * is max(1e-4, 2.5 * filter_err_a); a tolerance set here is kept as given, and if the model's
 * error floor does not fit under it the filter is switched off for this engine
 * (mjpl_info.filter_enabled = 0: everything runs on the float64 kernels). */
int mjpl_set_filter(mjpl_engine *e, int32_t enable, double tol);
/* how many items of the most recent launch went to the float64 kernel (synchronises) */
int64_t mjpl_filter_last_undecided(mjpl_engine *e);
/* diagnostic: the (edge, check index, geom a, geom b) records the last filter launch handed to the exact pair kernel;
 * returns how many there were (the arrays, each of `cap` entries or NULL, receive up to cap of them), or -1 */
int64_t mjpl_filter_undecided_pairs(mjpl_engine *e, int32_t *edge, int32_t *idx, int32_t *ga, int32_t *gb, int64_t cap);
/* The filter validates edges in two passes: the endpoints of all edges, then the interior
 * waypoints of the edges whose endpoint passed (MJPL_TWO_PASS=0 at create: one pass).  Returns how
 * many edges the interior pass of the most recent mjpl_check_edges* took (synchronises); 0 for a
 * one-pass launch, -1 if the filter is off. */
int64_t mjpl_filter_last_interior_edges(mjpl_engine *e);
/* The interior pass runs one lane per waypoint: a small kernel walks the waypoint recurrence of
 * every surviving edge once and writes the waypoints out as work items (MJPL_EXPAND=0 at create:
 * one lane per edge walks them; edges too long for the item space always do).  Returns how many
 * waypoint items the most recent mjpl_check_edges* checked (synchronises); -1 if never used. */
int64_t mjpl_filter_last_items(mjpl_engine *e);
/* The fused filter kernel spares an edge its waypoint checks when the END configuration keeps every enabled pair
 * farther apart than the pair can move while the planning joints travel the edge (a certificate that only ever says
 * "free": the verdict _valid_collision_interval, planning/utils.py:188-216, would reach by checking every waypoint).
 * Returns how many surviving edges of the most recent mjpl_check_edges* were spared (synchronises); -1 if the filter is off. */
int64_t mjpl_filter_last_certified(mjpl_engine *e);

/* ---- host-buffer entry points (stage H2D, run, copy back, synchronise) ---------- */

/* Batched CollisionConstraint.valid_config (collision_constraint.py:26-30):
 * valid[i] = 1 iff configuration i has no contact outside the allowed body pairs. */
int mjpl_check_configs(mjpl_engine *e, const double *Q, int64_t N, int32_t layout,
                       uint8_t *valid);

/* Batched "validated edge" of _constrained_extend (planning/utils.py:143-158): the endpoint
 * QB is collision-checked (check index 0), then the interior waypoints of
 * _valid_collision_interval(QA, QB, step_dist) (planning/utils.py:188-216) in order
 * (check index 1..K).  valid[e] = AND of all checks.  first_bad (nullable): -1 if valid,
 * else the index of the first failing check.  flags = MJPL_EDGE_INTERIOR_ONLY drops check 0,
 * which is _valid_collision_interval itself.  step_dist <= 0 -> MJPL_E_ARG
 * (the reference raises ValueError("`step_dist` must be > 0"), utils.py:207-208). */
int mjpl_check_edges(mjpl_engine *e, const double *QA, const double *QB, int64_t E,
                     double step_dist, int32_t layout, int32_t flags, uint8_t *valid,
                     int32_t *first_bad);

/* Batched mj_kinematics (call site collision_constraint.py:28) for the FK parity check:
 * xpos [N][nbody*3], xquat [N][nbody*4], geom_xpos [N][ngeom*3], geom_xmat [N][ngeom*9];
 * any output may be NULL. */
int mjpl_fk(mjpl_engine *e, const double *Q, int64_t N, int32_t layout,
            double *xpos, double *xquat, double *geom_xpos, double *geom_xmat);

/* ---- contacts: which geom pairs touch (data.contact.geom after mj_kinematics + mj_collision,
 * collision_constraint.py:26-30) -------------------------------------------------------------
 * Candidate pairs of mj_collision: every geom pair that passes contype/conaffinity, the weld-body
 * and parent-child filters, and has a collision function (all but plane-plane, plane-hfield).
 * Pairs the CollisionRuleset allows are INCLUDED, with allowed[p] = 1.  Order = the oracle's
 * enumeration order: g1 < g2 ascending, g2 ascending.  Each row is written smaller-geom-type first,
 * as orc_collision writes it.  The table is built at mjpl_create from the model alone;
 * mjpl_set_planning leaves it as it is.  mjpl_contact_pair_count returns P (>= 0) or < 0;
 * mjpl_contact_pairs fails with MJPL_E_ARG if cap < P or an output is NULL while P > 0. */
int32_t mjpl_contact_pair_count(mjpl_engine *e);
int mjpl_contact_pairs(mjpl_engine *e, int32_t *geom1, int32_t *geom2, uint8_t *allowed, int32_t cap);

/* bits[i * W + w] (W = (P + 63) / 64): bit (p % 64) of word p / 64 is set iff candidate pair p is
 * in contact at configuration i.  Exact float64 verdict with margin = max of the two margins: the
 * bound cull and narrowphase routine the collision check runs for that pair, so that
 * valid[i] of mjpl_check_configs == no set bit outside the allowed pairs.  Q as mjpl_check_configs
 * reads it: same layouts, same planning-joint selection.  P = 0: nothing is launched, MJPL_OK.
 * Non-finite entries of Q are not rejected, as in mjpl_check_configs: every pair is decided by the
 * same comparisons on the NaN / inf poses they produce (a comparison with NaN counts as contact
 * where the routine tests "not farther than", so such a configuration reports contacts and the
 * check calls it invalid).  MJPL_E_PAIRTYPE if a candidate pair has a geom type without a routine
 * here (only possible for allowed pairs: mjpl_create refuses the others).  The host-buffer form
 * synchronises; the device form is asynchronous on the engine's stream. */
int mjpl_contacts(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, uint64_t *bits);
int mjpl_contacts_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, uint64_t *dbits);

/* ---- distances and clearance: how far each configuration is from touching -------------------
 * Pair distance.  For candidate pair p of the contacts table (same P, same order, allowed pairs
 * included), d_p(q) is the exact geometric (Euclidean) signed distance of the two solids: the width
 * of the gap when they are disjoint (> 0), minus the penetration depth when they overlap (the length
 * of the shortest translation that separates them).  A plane is a half-space: d is the signed height
 * above it of the geom's lowest point (sphere centre - r, lower capsule end point - r, lowest box
 * corner).  Margins are NOT subtracted.  Float64 geometry, not the numbers of MuJoCo's convex solver.
 *
 * distmax (> 0, may be +inf): dist[i * P + p] = d_p(q_i) if d_p < distmax, else exactly distmax (the
 * contract of mj_geomDistance), which lets the kernel skip a pair whose bounding spheres (or centre
 * height above a plane minus geom_rbound) are distmax apart.
 *
 * Clearance.  clear[i] = min over NON-allowed p of (dist[i * P + p] - margin_p), margin_p =
 * max(m1, m2) as the check uses it; pair[i] = the candidate-table index of the minimiser, the lowest
 * on ties.  No non-allowed pair: clear = distmax, pair = -1.  With distmax > every margin,
 * clear[i] <= 0 <=> mjpl_check_configs calls q_i invalid, up to rounding at the threshold.
 *
 * A configuration with a non-finite planning column gives NaN in every dist[i * P + .] and clear[i],
 * and pair[i] = -1.  Q as mjpl_check_configs reads it: same layouts, same planning-joint selection.
 * N = 0, or P = 0 for mjpl_distances*, launches nothing and returns MJPL_OK.  MJPL_E_ARG: distmax NaN
 * or <= 0, a NULL output with N > 0, an unknown layout.  MJPL_E_PAIRTYPE as for mjpl_contacts.  The
 * results depend on no option and no MJPL_* variable.  The host-buffer forms synchronise; the device
 * forms are asynchronous on the engine's stream. */
int mjpl_distances(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax, double *dist);
int mjpl_distances_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax, double *ddist);
int mjpl_clearance(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax,
                   double *clear, int32_t *pair);
int mjpl_clearance_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax,
                       double *dclear, int32_t *dpair);

/* ---- clearance gradients and witness points ------------------------------------------------
 * clear[i] and pair[i] are bit-identical to what mjpl_clearance returns for the same Q, layout and
 * distmax.  Let p = pair[i] and (g1, g2) row p of mjpl_contact_pairs, in that row's orientation, and
 * D = clear[i] + margin_p the pair's signed distance.
 *   fromto[i*6 + 0..2] = w1, a point of g1; fromto[i*6 + 3..5] = w2, a point of g2 (world frame, the
 *     layout of mj_geomDistance's fromto).  Disjoint: closest points.  Overlap: the two ends of the
 *     shortest separating translation (along the separating axis that gave the depth).  Plane (always
 *     g1): w2 is the geom's lowest point, w1 its projection on the plane.
 *   normal[i*3 + 0..2] = n, the unit vector from g1 towards g2; w2 - w1 = D n up to rounding.
 *   grad[i*nplan + j] = d clear / d q_j over the planning columns of mjpl_set_planning, in its order:
 *     n . (v_j(w2 in body(g2)) - v_j(w1 in body(g1))), v_j(x) = axis_j x (x - anchor_j) for a hinge and
 *     axis_j for a slide (world frame after FK, the frame the joint moves), and v_j(x) = 0 unless the
 *     joint's body is the point's body or one of its ancestors (static geoms: 0).
 * Ties between pairs resolve to the lowest index, as for clear.  Where the clearance is not
 * differentiable (the closest pair or feature switches) the result is the one-sided gradient of the
 * pair and feature the kernel picked; it need not equal a central difference there.
 * status[i]:
 *   MJPL_GRAD_OK          all outputs set.
 *   MJPL_GRAD_FLAT        no non-allowed pair (pair = -1) or the winner is capped at distmax: grad
 *                         exactly 0, fromto and normal NaN.
 *   MJPL_GRAD_DEGENERATE  no normal can be formed: the disjoint core gap (closest points of the
 *                         sphere points, capsule segments and boxes before the radii) is below 1e-10,
 *                         e.g. crossing capsule axes: grad and normal NaN, fromto = the two core points.
 *   MJPL_GRAD_NONFINITE   a planning column is non-finite: everything NaN, clear NaN, pair -1.
 * fromto and normal may be NULL; every other output is required when N > 0.  N = 0 launches nothing.
 * Argument errors as mjpl_clearance (MJPL_E_ARG, MJPL_E_PAIRTYPE).  The results depend on no option and
 * no MJPL_* variable.  The host form synchronises; the device form is asynchronous on the engine's
 * stream. */
#define MJPL_GRAD_OK          0
#define MJPL_GRAD_FLAT        1
#define MJPL_GRAD_DEGENERATE  2
#define MJPL_GRAD_NONFINITE   3
int mjpl_clearance_grad(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax,
                        double *clear, int32_t *pair, double *grad, double *fromto, double *normal,
                        int32_t *status);
int mjpl_clearance_grad_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax,
                            double *dclear, int32_t *dpair, double *dgrad, double *dfromto, double *dnormal,
                            int32_t *dstatus);

/* ---- near pairs: every pair within distmax, with distance, witnesses and gradient ----------
 * Candidate pair p of the contacts table (same P, same order) is NEAR at q_i if it is not allowed and
 * d_p(q_i) < distmax: d_p is mjpl_distances' exact signed distance (margins not subtracted), and the
 * comparison is the one that decides whether mjpl_distances writes d_p or distmax.  Allowed pairs take
 * no part, as in mjpl_clearance.  K (>= 1) is the number of slots per configuration.
 *   count[i] = the number of near pairs of q_i, NOT clipped to K; -1 for a row with a non-finite
 *     planning column.
 *   Slots k < min(count[i], K) of row i hold the first near pairs in ascending p:
 *     pair[i*K + k] = p;  dist[i*K + k] = d_p, bit-identical to mjpl_distances.
 *   In every remaining slot of the row pair = -1 and NOTHING ELSE IS WRITTEN: dist, grad, fromto,
 *     normal and status keep the caller's bytes there.  Mask by pair (>= 0) or by count.
 * Per listed slot s = i*K + k, with (g1, g2) row p of mjpl_contact_pairs and D = dist[s]:
 *   fromto[s*6 + 0..5], normal[s*3 + 0..2] and grad[s*nplan + j] = d d_p / d q_j have the meaning,
 *     orientation and formula of the mjpl_clearance_grad block above for that pair (w1 on g1, w2 on g2,
 *     the plane and overlap cases, n from g1 towards g2, w2 - w1 = D n up to rounding, grad over the
 *     planning columns of mjpl_set_planning).  Where mjpl_clearance_grad picks pair p, its grad, fromto,
 *     normal and status are these, bit for bit.
 *   status[s] = MJPL_GRAD_OK or MJPL_GRAD_DEGENERATE, by the same rule and with the same outputs
 *     (DEGENERATE: grad and normal NaN, fromto = the two core points).  MJPL_GRAD_FLAT and
 *     MJPL_GRAD_NONFINITE do not occur per slot: a pair at or beyond distmax is not listed, and a
 *     non-finite row lists nothing.
 * Unlike the clearance's gradient, which follows one pair and flips where the winner switches, every
 * pair's own distance is listed with its own gradient: two walls at the same distance are two slots.
 * fromto and normal may be NULL; every other output is required when N > 0.  distmax > 0, +inf allowed.
 * MJPL_E_ARG: K < 1, distmax NaN or <= 0, an unknown layout, a NULL required output with N > 0.
 * MJPL_E_PAIRTYPE as for mjpl_contacts.  N = 0 launches nothing.  Without a non-allowed pair every
 * count is 0 (-1 for a non-finite row) and every pair -1.  The results depend on no option and no
 * MJPL_* variable.  The host form synchronises; the device form is asynchronous on the engine's
 * stream. */
int mjpl_near_pairs(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax, int32_t K,
                    int32_t *count, int32_t *pair, double *dist, double *grad, double *fromto, double *normal,
                    int32_t *status);
int mjpl_near_pairs_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax, int32_t K,
                        int32_t *dcount, int32_t *dpair, double *ddist, double *dgrad, double *dfromto,
                        double *dnormal, int32_t *dstatus);

/* ---- push out: move configurations to at least d_min from everything ----------------------
 * Q_out[i] is q_i moved until its clearance (mjpl_clearance: min over non-allowed pairs of
 * d_p - margin_p) is at least d_min, by damped least-squares steps on the near pairs' own gradients.
 * Parameters (mjpl_push_desc): d_min > 0; overshoot >= 0 (1e-3 is a good default); damping > 0
 * (1e-4); step_max > 0 (0.2); max_iter >= 1 (16); max_pairs K >= 1 (16); lo, hi: HOST arrays of
 * nplan bounds over the planning columns of mjpl_set_planning, either may be NULL (no bound), in
 * both forms of the call.
 *
 * M = the largest margin_p over the non-allowed candidate pairs (0 without one); D* = d_min + M is the
 * distmax of every measurement, taken once at the call.  Per row, from q = q_i:
 *   1. mjpl_near_pairs at q with distmax D* and K slots (no witnesses).
 *   2. Slot p is violated if dist_p - margin_p < d_min.
 *   3. A violated slot with status MJPL_GRAD_DEGENERATE ends the row as DEGENERATE; q is not moved.
 *   4. No violated slot: the row ends.
 *   5. Over the violated slots in ascending slot order: r_p = d_min + overshoot - (dist_p - margin_p),
 *      A = damping I + sum g_p g_p^T, b = sum r_p g_p, delta = A^-1 b by a Cholesky factorisation (A is
 *      positive definite because damping > 0).
 *   6. If s = max_j |delta_j| > step_max: delta <- delta * (step_max / s).
 *   7. q <- q + delta, then clamped to [lo, hi] where given.
 *   8. After max_iter steps without ending, the row ends as it stands.
 * Near but satisfied pairs take no part in a step; if a step pushes one into violation the next
 * iteration sees it.  Then ONE mjpl_clearance launch measures Q_out with distmax D* and fills clear
 * and pair: they are bit-identical to mjpl_clearance(Q_out, D*).  status[i] follows from that number
 * and nothing else:
 *   MJPL_PUSH_OK          clear[i] >= d_min.
 *   MJPL_PUSH_DEGENERATE  otherwise, if the row ended at step 3.
 *   MJPL_PUSH_STUCK       otherwise: also a d_min no configuration reaches, and a row whose violated
 *                         pairs lie beyond slot K.  Q_out is the last iterate.
 *   MJPL_PUSH_NONFINITE   a planning column is non-finite: Q_out = the caller's row, clear NaN, pair -1,
 *                         iters 0.
 * iters[i] = the number of steps taken.  A row that needs no push comes back byte for byte with
 * iters 0.  Q_out has the layout of Q.
 * A limit worth knowing: two geoms whose distance no planning column can open bound the clearance
 * from above.  In the Franka-P + 16 obstacles scene two non-allowed pairs of neighbouring links are
 * such: link0 - link1 stays at 0.033 m whatever the configuration and link1 - link3 never exceeds
 * 0.031 m, so no larger d_min is reached there and every row ends STUCK.
 * MJPL_E_ARG: a parameter outside its range, NaN in any parameter or bound, lo > hi in a column, a
 * NULL descriptor, a NULL output with N > 0, an unknown layout.  MJPL_E_PAIRTYPE as for
 * mjpl_near_pairs.  MJPL_E_CAPACITY: more than 16 planning columns, or none.  N = 0 launches nothing.
 * The results depend on no option and no MJPL_* variable.  The host form synchronises.  The device
 * form enqueues on the engine's stream but is NOT asynchronous: between iterations it synchronises
 * that stream to read how many rows are still active (4 bytes). */
#define MJPL_PUSH_OK          0
#define MJPL_PUSH_STUCK       1
#define MJPL_PUSH_DEGENERATE  2
#define MJPL_PUSH_NONFINITE   3
typedef struct {
  double d_min, overshoot, damping, step_max;
  int32_t max_iter, max_pairs;
  const double *lo, *hi; /* host, [nplan], may be NULL, both forms */
} mjpl_push_desc;
int mjpl_push_out(mjpl_engine *e, const mjpl_push_desc *desc, const double *Q, int64_t N, int32_t layout,
                  double *Q_out, double *clear, int32_t *pair, int32_t *iters, int32_t *status);
int mjpl_push_out_dev(mjpl_engine *e, const mjpl_push_desc *desc, const double *dQ, int64_t N, int32_t layout,
                      double *dQ_out, double *dclear, int32_t *dpair, int32_t *diters, int32_t *dstatus);

/* ---- trajectories: time-optimal parameterisation of a batch of paths -----------------------
 * A path is n >= 2 waypoints of nq columns (1..16); B paths are packed one after another in W, path b
 * being rows wp_off[b] .. wp_off[b+1] - 1 (wp_off[0] = 0).  mjpl_topp_profile finds, per path, the fastest
 * motion along the natural cubic spline through its waypoints under per-column limits
 * vmin < 0 < vmax on velocity and amin < 0 < amax on acceleration (mjpl_topp_desc: HOST arrays of nq
 * entries, in both forms of the calls; grid >= 2 intervals per waypoint segment, 8 is a good default).
 * The engine gives its device, stream and staging slots; its model plays no part.
 *
 * Per path (tests/trajectory_reference.py states every operation; DESIGN.md section 5.12 derives it):
 *   1. M[n][nq], the knot second derivatives of the natural spline at the knots s_k = k / (n-1)
 *      (zero at both ends), by the Thomas recurrence per column.
 *   2. A grid of N = (n-1) * grid intervals of width D = 1/N; a_i = q'(s_i), b_i = q''(s_i).
 *   3. x_i = sdot^2 at grid point i, x_0 = x_N = 0; u_i = sddot on interval i, x_{i+1} = x_i + 2 D u_i.
 *   4. Interval i: x_i <= min_j (v*_j / a_ij)^2 (v* = vmax where a_ij > 0, vmin where < 0); and per column at
 *      BOTH ends of the interval amin_j <= a_ij u + b_ij x_i <= amax_j and
 *      amin_j <= (a_{i+1,j} + 2 D b_{i+1,j}) u + b_{i+1,j} x_i <= amax_j (the second is the acceleration at
 *      the right end with x_{i+1} written out); and 0 <= x_i + 2 D u <= K_{i+1}.  All are lines in (u, x).
 *   5. Backward: K_N = 0, K_i = the largest x_i for which some u satisfies all of 4 = max(0, the least
 *      intersection of a lower with an upper line), in closed form.
 *   6. Forward: u_i = the largest u the upper lines allow at x_i, x_{i+1} = clamp(x_i + 2 D u_i, 0, K_{i+1});
 *      then u_i = (x_{i+1} - x_i) / 2D.
 *   7. t_0 = 0, t_{i+1} = t_i + 2 D / (sqrt x_i + sqrt x_{i+1}).
 * Outputs: M like W; x, u, t packed at g_off[b] = grid (wp_off[b] - b) + b with N_b + 1 entries per path,
 * u's last entry 0, t's last entry the duration.  status[b]:
 *   MJPL_TOPP_OK         otherwise.  A single interior x_i = 0 is a stop, and OK.
 *   MJPL_TOPP_STALLED    two consecutive x_i are 0: that interval takes for ever (t holds inf from there).
 *   MJPL_TOPP_NONFINITE  a waypoint of the path holds NaN / inf: its M, x, u, t are NaN -- or a result is
 *                        not finite.  Other paths of the batch are not affected.
 * Two consecutive equal waypoints are not refused here (the Python binding raises ValueError).
 *
 * mjpl_topp_sample evaluates the motion: path b gets samp_off[b+1] - samp_off[b] samples (samp_off[0] = 0,
 * non-decreasing), sample k = 1, 2, ... at t_k = min(k dt, duration).  The caller sizes them: m =
 * ceil((duration - 1e-8) / dt) puts the last sample at the duration itself, where the position is the last
 * waypoint and the velocity 0.  In the interval t_i <= t_k <= t_{i+1}, tau = t_k - t_i:
 *   sdot = sqrt x_i + u_i tau,  s = s_i + sqrt x_i tau + u_i tau^2 / 2,
 *   pos = q(s),  vel = q'(s) sdot,  acc = q''(s) sdot^2 + q'(s) u_i,     each [samp_off[B]][nq].
 * Sampling a path that is not OK reads NaN / inf times and gives meaningless rows, never a fault.
 *
 * wp_off and samp_off are HOST arrays in both forms.  MJPL_E_ARG: a NULL pointer, grid < 2, a path with
 * fewer than 2 waypoints or offsets that fall, a limit of the wrong sign, infinite or NaN, dt <= 0 or
 * NaN.  MJPL_E_CAPACITY: nq outside 1..16, a path of more than 2^24 grid points.  B = 0 (and a sample call
 * without samples) launches nothing.  All outputs are deterministic and depend on no option and no MJPL_*
 * variable: the option "topp_chunk_bytes" (the workspace of one chunk of paths, 512 MiB) changes the number
 * of launches -- "topp_last_chunks" reads it back -- and no bit of any output.  The host forms synchronise.  The device forms synchronise the engine's stream once on entry
 * (before the offset tables of an earlier call are replaced) and return with their launches enqueued. */
#define MJPL_TOPP_OK         0
#define MJPL_TOPP_STALLED    1
#define MJPL_TOPP_NONFINITE  2
typedef struct {
  int32_t nq, grid;
  const double *vmin, *vmax, *amin, *amax; /* host, [nq], both forms */
} mjpl_topp_desc;
int mjpl_topp_profile(mjpl_engine *e, const mjpl_topp_desc *desc, const double *W, const int64_t *wp_off, int64_t B,
                      double *M, double *x, double *u, double *t, int32_t *status);
int mjpl_topp_profile_dev(mjpl_engine *e, const mjpl_topp_desc *desc, const double *dW, const int64_t *wp_off,
                          int64_t B, double *dM, double *dx, double *du, double *dt, int32_t *dstatus);
int mjpl_topp_sample(mjpl_engine *e, const mjpl_topp_desc *desc, const double *W, const int64_t *wp_off, int64_t B,
                     const double *M, const double *x, const double *u, const double *t, double dt,
                     const int64_t *samp_off, double *pos, double *vel, double *acc);
int mjpl_topp_sample_dev(mjpl_engine *e, const mjpl_topp_desc *desc, const double *dW, const int64_t *wp_off,
                         int64_t B, const double *dM, const double *dx, const double *du, const double *dt_grid,
                         double dt, const int64_t *samp_off, double *dpos, double *dvel, double *dacc);

/* ---- trajectories: jerk-limited parameterisation of a batch of paths -----------------------
 * The same paths, packing, spline and engine as mjpl_topp_* above, under per-column limits on velocity,
 * acceleration AND jerk (mjpl_jerk_desc: HOST arrays of nq magnitudes > 0, in both forms of the calls;
 * grid >= 1 intervals per waypoint segment, 2 is a good default).  The motion passes through the waypoints
 * without stopping; it is not time-optimal (DESIGN.md section 5.14 says by how much).  Every column's
 * velocity, acceleration and jerk stay within their limits at every instant, not only at grid points.
 *
 * Per path (tests/jerk_reference.py states every operation; DESIGN.md section 5.14 proves the guarantee):
 *   1. M as mjpl_topp_profile's, bit for bit.  A grid of N = (n-1) * grid intervals of width D = 1/N; the
 *      grid points are the junctions.
 *   2. Interval i, column j: p1 = max |q'|, p2 = max |q''|, p3 = |q'''| over the interval, exactly (q' at both
 *      ends and at its vertex if that lies inside, q'' at both ends, q''' is constant).
 *   3. The interval's limits on sdot, |sddot|, |sdddot| (a term with a zero denominator is +inf):
 *        V_i = min_j min(v_j / p1, sqrt(a_j / (2 p2)), cbrt(j_j / (3 p3)))
 *        A_i = min_j min((a_j - p2 V_i^2) / p1, j_j / (9 p2 V_i))
 *        J_i = min_j (j_j - p3 V_i^3 - 3 p2 V_i A_i) / p1.
 *   4. A ramp changes the speed by dv with sddot = 0 at both ends in T(dv) = dv/A + A/J if dv >= A^2/J, else
 *      2 sqrt(dv/J), over the length (v0 + v1)/2 T(dv).
 *   5. Junction speeds v_i (sddot = 0 there): v_0 = v_N = 0, v_i <= min(V_{i-1}, V_i); backward, v_i is no
 *      faster than a ramp down to v_{i+1} within D allows; forward, v_{i+1} no faster than a ramp up from v_i.
 *      The largest such speed is found by a section search: ten rounds of 64 candidates, always feasible.
 *   6. Interval i: ramp from v_i up to the peak vp_i (the largest <= V_i whose two ramps fit D, by the same
 *      search), cruise for tc_i = (D - their length) / vp_i, ramp down to v_{i+1}: seven phases of constant
 *      sdddot (J, 0, -J, 0, -J, 0, J), some of zero length.
 *   7. t_0 = 0, t_{i+1} = t_i + ((T_up + tc_i) + T_down).
 * Outputs: M like W; v, vp, tc, t packed at g_off[b] = grid (wp_off[b] - b) + b with N_b + 1 entries per
 * path (vp's and tc's last entry 0, t's last entry the duration); lim with N_b + 1 rows (V, A, J) per path
 * at 3 g_off[b], the last row 0.  status[b], numerically mjpl_topp_profile's:
 *   MJPL_TOPP_OK         otherwise.
 *   MJPL_TOPP_STALLED    some V_i is +inf: nothing moves on that interval.  v and vp are 0, tc and t +inf
 *                        (t_0 = 0).
 *   MJPL_TOPP_NONFINITE  a waypoint of the path holds NaN / inf, or a result is not finite: its M, lim, v, vp,
 *                        tc, t are NaN.  Other paths of the batch are not affected.
 *
 * mjpl_jerk_sample evaluates the motion at mjpl_topp_sample's times and counts.  In the interval
 * t_i <= t_k, tau = t_k - t_i, the phases are walked from (s, sdot, sddot) = (0, v_i, 0) to the one that
 * holds tau; at or past t_{i+1} - t_i the state is (D, v_{i+1}, 0).  Then pos = q(s), vel = q'(s) sdot,
 * acc = q''(s) sdot^2 + q'(s) sddot: the last sample is the last waypoint, at rest.  Sampling a path that is
 * not OK gives meaningless rows, never a fault.
 *
 * wp_off and samp_off are HOST arrays in both forms.  MJPL_E_ARG: a NULL pointer, grid < 1, a path with
 * fewer than 2 waypoints or offsets that fall, a limit that is not > 0, infinite or NaN, dt <= 0 or NaN.
 * MJPL_E_CAPACITY: nq outside 1..16, a path of more than 2^24 grid points.  B = 0 (and a sample call without
 * samples) launches nothing.  All outputs are deterministic and depend on no option and no MJPL_* variable;
 * there is no workspace.  The host forms synchronise.  The device forms synchronise the engine's stream
 * once on entry and return with their launches enqueued. */
typedef struct {
  int32_t nq, grid;
  const double *vlim, *alim, *jlim; /* host, [nq], both forms */
} mjpl_jerk_desc;
int mjpl_jerk_profile(mjpl_engine *e, const mjpl_jerk_desc *desc, const double *W, const int64_t *wp_off, int64_t B,
                      double *M, double *lim, double *v, double *vp, double *tc, double *t, int32_t *status);
int mjpl_jerk_profile_dev(mjpl_engine *e, const mjpl_jerk_desc *desc, const double *dW, const int64_t *wp_off,
                          int64_t B, double *dM, double *dlim, double *dv, double *dvp, double *dtc, double *dt,
                          int32_t *dstatus);
int mjpl_jerk_sample(mjpl_engine *e, const mjpl_jerk_desc *desc, const double *W, const int64_t *wp_off, int64_t B,
                     const double *M, const double *lim, const double *v, const double *vp, const double *tc,
                     const double *t, double dt, const int64_t *samp_off, double *pos, double *vel, double *acc);
int mjpl_jerk_sample_dev(mjpl_engine *e, const mjpl_jerk_desc *desc, const double *dW, const int64_t *wp_off,
                         int64_t B, const double *dM, const double *dlim, const double *dv, const double *dvp,
                         const double *dtc, const double *dt_grid, double dt, const int64_t *samp_off, double *dpos,
                         double *dvel, double *dacc);

/* ---- path shortcutting: many paths in lockstep, one edge launch per round ---------------------
 * The B paths are packed as for mjpl_topp_*: rows W[wp_off[b] .. wp_off[b+1] - 1], each of as many columns
 * as the engine's planning set (mjpl_set_planning; the full nq by default).  mjpl_shortcut_paths removes
 * waypoints: wherever the straight edge between two waypoints of a path passes mjpl_check_edges and is
 * shorter than the stretch between them.  Every number and decision below is stated in NumPy by
 * tests/shortcut_reference.py; the kernels (mjpl_amd/csrc/mjpl_shortcut.h) match it bit for bit.
 *
 * d(a, b) = sqrt(sum_c (W[b][c] - W[a][c])^2), the columns added in order from 0.0, one IEEE rounding per
 * operation.  A path's live list starts as all its rows.  A path with a NaN or inf anywhere gets status
 * NONFINITE and is left alone (keep all 1, n_out its row count, length NaN, proposed = accepted = 0).
 * For round r = 0 .. rounds - 1, for every path b (its index in the call) not yet retired, of m live waypoints:
 *   1. m <= 2: status CONVERGED, retired.
 *   2. L[0] = 0, L[k] = L[k-1] + d(live[k-1], live[k]), added in index order.
 *   3. npairs = (m-1)(m-2)/2; the round is exhaustive iff npairs <= candidates.  Candidate l < candidates is,
 *      in an exhaustive round, the l-th pair (i, j), j >= i + 2, in lexicographic order (none for l >= npairs);
 *      otherwise z = sm(sm(sm(seed) ^ b) ^ (64 r + l)), sm = splitmix64's step (x += 0x9E3779B97F4A7C15;
 *      x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^= x >> 31; mod 2^64),
 *      i = ((z & 0xffffffff) (m-2)) >> 32, j = i + 2 + (((z >> 32) (m-2-i)) >> 32).  Its saving is
 *      s = (L[j] - L[i]) - d(live[i], live[j]); it is PROPOSED iff s > min_saving.
 *   4. The verdict of a proposed candidate is mjpl_check_edges(QA = W[live[i]], QB = W[live[j]], step_dist,
 *      flags = 0) -- every proposal of every path in ONE launch of the edge pipeline per round; an edge the
 *      edge kernels refuse (first_bad = -2) counts as invalid, and no MJPL_E_NONFINITE is reported for it.
 *   5. An exhaustive round without a valid proposal: status CONVERGED, retired -- at the sampled verdict no
 *      single shortcut of the path is both valid and shorter.
 *   6. The valid proposals, by (s descending, l ascending): one is accepted iff it is compatible with every
 *      one accepted before it ((i, j) and (i', j') are compatible iff j <= i' or j' <= i); live[i+1 .. j-1]
 *      of every accepted one leave the list.  Comparisons only.
 * Paths not retired after the last round get status ROUNDS.  keep [wp_off[B]]: 1 = the row survives (the
 * first and last row of a path always do); n_out [B] the survivors; length [B] is L over the final live
 * list; proposed [B] the edges validated, accepted [B] the shortcuts taken.  length, proposed and accepted
 * may be NULL.  The state after `rounds` = R equals the state of a longer run after R rounds.
 *
 * MJPL_E_ARG: a NULL pointer, step_dist <= 0 or NaN, rounds < 1, candidates outside 1..64, min_saving
 * negative or NaN, a path of fewer than 2 rows (offsets that fall included); MJPL_E_CAPACITY: a path of more
 * than 65 536 rows.  B = 0 launches nothing.  The option "shortcut_chunk_bytes" (the workspace of one chunk
 * of paths, 256 MiB) changes the number of launches -- "shortcut_last_chunks" reads it back -- and no bit of
 * any output.  Both forms synchronise the engine's stream once per round (the round's edge count comes
 * back to the host); wp_off is a host array in both.  The edge pipeline's status word (mjpl_take_status)
 * is cleared by the call. */
#define MJPL_SHORTCUT_CONVERGED 0
#define MJPL_SHORTCUT_ROUNDS    1
#define MJPL_SHORTCUT_NONFINITE 2
typedef struct {
  double step_dist, min_saving;
  uint64_t seed;
  int32_t rounds, candidates;
} mjpl_shortcut_desc;
int mjpl_shortcut_paths(mjpl_engine *e, const mjpl_shortcut_desc *desc, const double *W, const int64_t *wp_off, int64_t B,
                        uint8_t *keep, int32_t *n_out, double *length, int32_t *status, int32_t *proposed,
                        int32_t *accepted);
int mjpl_shortcut_paths_dev(mjpl_engine *e, const mjpl_shortcut_desc *desc, const double *dW, const int64_t *wp_off,
                            int64_t B, uint8_t *dkeep, int32_t *dn_out, double *dlength, int32_t *dstatus,
                            int32_t *dproposed, int32_t *daccepted);

/* ---- planning: many start/goal pairs in lockstep, one edge launch per round --------------------
 * A bidirectional RRT over B independent problems that all take their rounds together: the planner for many
 * mostly easy queries (mjpl_rrt_* stays the one for a single hard query).  QI, QG [B][nplan] are the ends, over
 * the engine's planning columns (mjpl_set_planning; the full nq by default); lo, hi [nplan] the sampling box,
 * HOST arrays in both forms.  Every number and decision below is stated in NumPy by tests/plan_reference.py;
 * the kernels (mjpl_amd/csrc/mjpl_plan.h) match it bit for bit.
 *
 * d2(a, t) = sum_c (t[c] - a[c])^2, the columns added in order from 0.0, one IEEE rounding per operation.
 * step(a, t): m = sqrt(d2(a, t)); t itself if m <= epsilon, otherwise column c is
 * a[c] + ((t[c] - a[c]) / m) * epsilon.  nearest(T, t) is the lowest index k that minimises d2(T[k], t).
 * sm is splitmix64's step (see mjpl_shortcut_paths).
 *
 * Ends.  1. A problem with a NaN or inf in either end gets status NONFINITE.  2. One configuration launch
 * (mjpl_check_configs) validates all remaining ends; a problem with an invalid end gets INVALID_END.  3. One
 * edge launch validates the direct edges QA = QI[b], QB = QG[b]; a valid one gives SOLVED, the path
 * [QI[b], QG[b]] and rounds_used = 0.  4. Otherwise T0 = {QI[b]}, T1 = {QG[b]}, both of parent -1, gained = 0.
 *
 * Round r = 0 .. rounds - 1, for every live problem b (its index in the call):
 *   1. Tree g = r & 1 grows, o = 1 - g is the other; n_g, n_o are their sizes at the start of the round.
 *   2. n_g >= nodes: status NODES, rounds_used = r, retired.
 *   3. The connect candidate exists only if gained > 0: for each p among the last `gained` nodes of T_o (those
 *      it gained in round r - 1), n = nearest(T_g, T_o[p]); the pair of the least d2 wins, ties to the lowest
 *      p; the connect edge is QA = T_o[p], QB = T_g[n].
 *   4. Extension candidates l < min(candidates, nodes - n_g): z = sm(sm(sm(seed) ^ b) ^ (64 r + l)); for
 *      c = 0 .. nplan - 1: u = (z >> 11) * 2^-53, t[c] = lo[c] + u * (hi[c] - lo[c]), z = sm(z);
 *      k = nearest(T_g, t), q = step(T_g[k], t); the extension edge is QA = T_g[k], QB = q.
 *   5. ONE launch of the edge pipeline validates every edge of every problem (per problem: the connect edge,
 *      then the extensions in order of l), at step_dist, flags 0: the verdicts of mjpl_check_edges on the
 *      same rows.  An edge the edge kernels refuse counts as invalid, and no MJPL_E_NONFINITE is reported.
 *   6. A valid connect edge: SOLVED, rounds_used = r + 1, this round's extensions dropped; the path is T0 from
 *      its root to its junction node, then T1 from its junction node to its root, nothing de-duplicated.
 *      Otherwise the valid extensions are appended to T_g in order of l with parent k, and gained = their count.
 * Problems live after the last round get ROUNDS, rounds_used = rounds.  A tree's depth is at most the number
 * of rounds it grew in, so a path has at most rounds + 2 rows.
 *
 * P [B][rounds + 2][nplan]: rows 0 .. n_out - 1 are the path of a SOLVED problem (first and last row bit-equal
 * to the ends), every other row is zero; n_out [B] (0 unless SOLVED); status [B]; and, each may be NULL,
 * rounds_used [B], edges [B] (edges validated for the problem, the direct one included), tree_nodes [B][2]
 * (the sizes of T0 and T1; 0 0 for a problem that never reached step 4).  The state after `rounds` = R
 * equals the state of a longer run after R rounds.
 *
 * MJPL_E_ARG: a NULL required pointer, epsilon or step_dist <= 0 or NaN, rounds outside 1..4096, candidates
 * outside 1..64, nodes outside 2..65536, a non-finite lo or hi (or width hi - lo), lo[c] > hi[c], B < 0.
 * B = 0 launches nothing.  The option "plan_chunk_bytes" (the workspace of one chunk of problems, 256 MiB)
 * changes the number of launches -- "plan_last_chunks" reads it back -- and no bit of any output.  Both
 * forms synchronise the engine's stream once per round (the round's edge count comes back to the host).
 * The edge pipeline's status word (mjpl_take_status) is cleared by the call. */
#define MJPL_PLAN_SOLVED      0
#define MJPL_PLAN_ROUNDS      1
#define MJPL_PLAN_NONFINITE   2
#define MJPL_PLAN_INVALID_END 3
#define MJPL_PLAN_NODES       4
typedef struct {
  double epsilon, step_dist;
  uint64_t seed;
  int32_t rounds, candidates, nodes, reserved;
} mjpl_plan_desc;
int mjpl_plan_paths(mjpl_engine *e, const mjpl_plan_desc *desc, const double *QI, const double *QG, int64_t B,
                    const double *lo, const double *hi, double *P, int32_t *n_out, int32_t *status,
                    int32_t *rounds_used, int32_t *edges, int32_t *tree_nodes);
int mjpl_plan_paths_dev(mjpl_engine *e, const mjpl_plan_desc *desc, const double *dQI, const double *dQG, int64_t B,
                        const double *lo, const double *hi, double *dP, int32_t *dn_out, int32_t *dstatus,
                        int32_t *drounds_used, int32_t *dedges, int32_t *dtree_nodes);

/* ---- planning under a PoseConstraint: many start/goal pairs in lockstep, every edge a projected step ----
 * mjpl_plan_paths consults the collision check only, and joins its trees by one straight edge of any length --
 * an edge whose interior leaves a constraint manifold.  These two calls plan under the PoseConstraint of a pose
 * handle `p` (mjpl_pose_create), enforced by projection as the reference's CBiRRT does: every tree edge is ONE
 * projected step of at most epsilon, and the trees are joined by a BRIDGE -- a chain of projected steps from the
 * growing tree towards the other tree, closed by a straight edge of at most epsilon.  The engine is the handle's
 * engine; QI, QG, lo, hi, the planning columns and the lockstep of the rounds are those of mjpl_plan_paths.
 * Every number and decision below is stated in NumPy by tests/cplan_reference.py; the kernels
 * (mjpl_amd/csrc/mjpl_cplan.h) match it bit for bit.
 *
 * d2, step(a, t) with epsilon, nearest, sm, the sample t of (seed, b, r, l) and the box lo, hi: as for
 * mjpl_plan_paths.  New:
 *   project(a, x) -> (y, ok), over planning rows: a and x are expanded to full qpos rows (qpos_base with the
 *     planning columns replaced); the handle's PoseConstraint.apply runs on x with q_old = a -- the results of
 *     mjpl_pose_apply on the same rows; ok = 0 if the projection reports failure (joint limits left, farther
 *     than 2 q_step from q_old, the iteration bound reached), and also if any non-planning column of the
 *     result differs in bits from qpos_base; y is the planning columns of the result.
 *   cstep(a, t): x = step(a, t), (y, ok) = project(a, x).  Void if !ok, or sqrt(d2(a, y)) < 1e-8, or
 *     d2(y, t) > d2(a, t) (the three termination rules of the reference's _constrained_extend); otherwise y.
 *
 * Ends.  1. A problem with a NaN or inf in either end gets status NONFINITE.  2. One configuration launch
 * (mjpl_check_configs) and one mjpl_pose_valid launch cover all remaining ends; an end that fails either gives
 * INVALID_END.  3. Every other problem starts with T0 = {QI[b]}, T1 = {QG[b]}, both of parent -1, gained = 0.
 * There is no separate direct-edge stage: round 0's bridge covers it.
 *
 * Round r = 0 .. rounds - 1, for every live problem b (its index in the call):
 *   1. Tree g = r & 1 grows, o = 1 - g is the other; n_g, n_o are their sizes at the start of the round.
 *      n_g >= nodes: status NODES, rounds_used = r, retired.
 *   2. Bridge target: for each p among the last max(1, gained) nodes of T_o, n = nearest(T_g, T_o[p]); the pair
 *      of the least d2 wins, ties to the lowest p.  t = T_o[p], c_0 = T_g[n].
 *   3. Bridge chain, s = 1 .. min(chain, nodes - n_g): if sqrt(d2(c_{s-1}, t)) <= epsilon the chain ends with
 *      the CLOSING EDGE QA = c_{s-1}, QB = t.  Otherwise y = cstep(c_{s-1}, t); a void y ends the chain; else
 *      c_s = y is a LINK with the edge QA = c_{s-1}, QB = c_s.  `links` is the number of links.  The chain is
 *      generated before any verdict: a projection depends on the projected row before it, not on that row's
 *      collision verdict.
 *   4. Extension candidates l < min(candidates, nodes - n_g - links): t_l drawn as in mjpl_plan_paths,
 *      k = nearest(T_g, t_l) over the tree as it stood at the start of the round, y = cstep(T_g[k], t_l).  A
 *      void candidate sends no edge and is not counted; otherwise its edge is QA = T_g[k], QB = y.
 *   5. ONE launch of the edge pipeline validates every edge of every problem (per problem: the links, the
 *      closing edge if there is one, the non-void extensions in order of l), at step_dist, flags 0, exactly as
 *      mjpl_plan_paths does: a refused edge counts as invalid.  A round in which no problem has an edge
 *      launches nothing.
 *   6. The leading valid links are appended to T_g: the first with parent n, each following one with the link
 *      before it as parent.  If a closing edge exists, every link was valid and the closing edge is valid:
 *      SOLVED, rounds_used = r + 1, the junctions are the last appended link (n when there is no link) and
 *      T_o[p], this round's extensions dropped.  Otherwise the valid extensions are appended in order of l with
 *      parent k.  In both cases gained = the number of nodes appended this round.
 *   7. The path of a SOLVED problem is T0 from its root to its junction, then T1 from its junction to its root,
 *      nothing de-duplicated.  A path of more than max_rows rows: status LONG, n_out = 0.
 * Problems live after the last round get ROUNDS, rounds_used = rounds.  The state after `rounds` = R equals
 * the state of a longer run after R rounds.
 *
 * P [B][max_rows][nplan], zeroed by the call: rows 0 .. n_out - 1 are the path of a SOLVED problem (first and
 * last row bit-equal to the ends); n_out [B] (0 unless SOLVED); status [B]; and, each may be NULL,
 * rounds_used [B], edges [B] (edges validated for the problem), tree_nodes [B][2] (0 0 for NONFINITE and
 * INVALID_END).  Every row of a path is a projection's result or an end that passed mjpl_pose_valid; the
 * interior of a step is sampled for collision only, as in the reference.
 *
 * MJPL_E_ARG: everything mjpl_plan_paths refuses, chain outside 1..32, max_rows < 2, a NULL handle, more
 * planning columns than the projection's 16.  (The call knows the handle's engine only: a binding that takes an
 * engine AND a handle refuses a handle of another engine itself, as mjpl_amd's does with a ValueError.)  The options "plan_chunk_bytes" (no bit of any
 * output changes) and the read-only "plan_last_chunks", "plan_last_rounds", "plan_last_edges" serve these calls
 * as they serve mjpl_plan_paths; with "kernel_timer" & 1, "plan_last_project_ms" is the projections' share.
 * Choose epsilon < 2 q_step: at epsilon = 2 q_step the projection's "farther than 2 q_step" rule turns on
 * roundings. */
#define MJPL_PLAN_LONG        5
typedef struct {
  double epsilon, step_dist;
  uint64_t seed;
  int32_t rounds, candidates, nodes, chain, max_rows, reserved;
} mjpl_cplan_desc;
struct mjpl_pose; /* (mjpl_pose_create, below) */
int mjpl_plan_paths_constrained(struct mjpl_pose *p, const mjpl_cplan_desc *desc, const double *QI, const double *QG,
                                int64_t B, const double *lo, const double *hi, double *P, int32_t *n_out,
                                int32_t *status, int32_t *rounds_used, int32_t *edges, int32_t *tree_nodes);
int mjpl_plan_paths_constrained_dev(struct mjpl_pose *p, const mjpl_cplan_desc *desc, const double *dQI,
                                    const double *dQG, int64_t B, const double *lo, const double *hi, double *dP,
                                    int32_t *dn_out, int32_t *dstatus, int32_t *drounds_used, int32_t *dedges,
                                    int32_t *dtree_nodes);

/* ---- chained extensions: an extension candidate is a chain of up to `extend` projected steps ----
 * In the rounds above an extension is ONE step of epsilon, so a tree's frontier moves by at most epsilon a round.
 * The reference's _constrained_extend runs towards its target until it is stopped; these two calls take that
 * loop inside one round and cut it at `extend` (X, 1..32) steps.  The descriptor and every other argument are
 * those of mjpl_plan_paths_constrained*, which are these calls with extend = 1, bit for bit.
 * tests/cplan_extend_reference.py is the NumPy statement.  The round stays as written except for steps 4 to 6:
 *   4. The candidates are, as above, l < nc = min(candidates, nodes - n_g - links); t_l and k = nearest(T_g, t_l)
 *      are taken, as above, over the tree as it stood at the start of the round.  Candidate l has an extension
 *      chain: x_0 = T_g[k], and for s = 1 .. X, y = cstep(x_{s-1}, t_l).  A void y ends the chain; otherwise
 *      x_s = y is an extension link with the edge QA = x_{s-1}, QB = x_s.  There is no rule for reaching the
 *      target: at the target cstep moves less than 1e-8 and is void, which is how the reference's loop ends
 *      too.  A chain with no link sends no edge.  As for the bridge, a chain is generated before any verdict.
 *   5. The one edge launch takes, per problem, the bridge links, then the closing edge, then, for l ascending,
 *      chain l's links for s ascending.
 *   6. When the problem is not SOLVED the chains are appended for l ascending, and within a chain its leading
 *      valid links in order of s: the first link's parent is k, each later link's the link before it.  A link
 *      is appended only while the growing tree has fewer than `nodes` nodes; the first link of a chain that is
 *      invalid, or that meets a full tree, ends that chain's appending.  gained = the nodes appended in the
 *      round, bridge links included (at most chain + 64 X: the bridge target of step 2 is sought among them).
 * With X = 1 this is the text above: nc <= nodes - n_g - links, so the cap never bites.  A chunk's workspace
 * ("plan_chunk_bytes") holds chain + 1 + candidates X edges and 64 X chain rows per problem.
 * MJPL_E_ARG: extend outside 1..32, checked before anything else (with B = 0 too); then as above. */
int mjpl_plan_paths_constrained_ext(struct mjpl_pose *p, const mjpl_cplan_desc *desc, int32_t extend,
                                    const double *QI, const double *QG, int64_t B, const double *lo,
                                    const double *hi, double *P, int32_t *n_out, int32_t *status,
                                    int32_t *rounds_used, int32_t *edges, int32_t *tree_nodes);
int mjpl_plan_paths_constrained_ext_dev(struct mjpl_pose *p, const mjpl_cplan_desc *desc, int32_t extend,
                                        const double *dQI, const double *dQG, int64_t B, const double *lo,
                                        const double *hi, double *dP, int32_t *dn_out, int32_t *dstatus,
                                        int32_t *drounds_used, int32_t *dedges, int32_t *dtree_nodes);

/* ---- roadmap planning: validate a scene's edges once, answer many queries ------------------------
 * mjpl_plan_paths keeps nothing between calls: every call validates its edges again in the same static scene.
 * These two calls are the multi-query form (a probabilistic roadmap).  mjpl_roadmap_build turns N configurations
 * into a graph of validated edges, written into the CALLER's arrays; mjpl_roadmap_query reads those arrays and
 * answers B start/goal pairs with one configuration launch, ONE edge launch and a shortest-path search.  The
 * engine keeps no roadmap: a graph is valid for the scene and planning columns it was built with, and it is the
 * caller who keeps them together.  Every number and decision below is stated in NumPy by
 * tests/roadmap_reference.py; the kernels (mjpl_amd/csrc/mjpl_roadmap.h) match it bit for bit.
 *
 * d2(a, t) = sum_c (t[c] - a[c])^2, the columns added in order from 0.0, one IEEE rounding per operation (as for
 * mjpl_plan_paths); d2(a, t) and d2(t, a) are the same bits.  r2 = radius * radius; lo2 = r2 * 2^-40 (exact).
 *
 * mjpl_roadmap_build.  Q [N][nplan] over the engine's planning columns.  Outputs node_valid [N], row_off [N + 1],
 * adj [2 N k], w [2 N k].
 *   1. Nodes.  A row with a NaN or inf is invalid; one configuration launch (mjpl_check_configs; zeros stand in for
 *      such a row) gives the validity of every other row.
 *   2. Neighbours.  For each valid i, knn(i) is the first k by ascending (d2, j) of the valid j != i with
 *      lo2 <= d2(Q[i], Q[j]) <= r2: ties go to the lowest index.  The lower bound keeps coincident and
 *      near-coincident nodes apart: every weight is at least 2^-20 radius, so with N <= 2^20 every path length
 *      L <= 2^21 radius has fl(L + w) > L, on which step 4 of the query relies.
 *   3. Candidate edges: the pairs i < j with j in knn(i) or i in knn(j), each once, in ascending (i, j); the edge
 *      is QA = Q[i], QB = Q[j].  The edge pipeline validates them at step_dist, flags 0 (the verdicts of
 *      mjpl_check_edges on the same rows; an edge the edge kernels refuse counts as invalid, and no
 *      MJPL_E_NONFINITE is reported), in as many launches as the option "roadmap_chunk_bytes" asks for.
 *   4. Graph: a symmetric CSR adjacency.  Entries row_off[v] .. row_off[v + 1] - 1 of adj hold the other endpoint of
 *      each valid edge at v, ascending by node index; w holds sqrt(d2) of the edge (the same bits in both rows).
 *      Entries at and past row_off[N] are adj = -1, w = 0.
 * MJPL_E_ARG: a NULL required pointer, radius or step_dist <= 0, NaN or inf, k outside 1..32, N outside 0..2^20.
 * N = 0 launches nothing and writes nothing (the empty graph is row_off[0] = 0).
 *
 * mjpl_roadmap_query.  The graph arrays as built, and QI, QG [B][nplan].  Outputs P [B][max_rows][nplan] (zeroed by
 * the call; rows 0 .. n_out - 1 are the path), n_out [B], status [B] and cost [B] (may be NULL; 0.0 unless SOLVED).
 *   1. Ends.  A NaN or inf in either end: NONFINITE.  Otherwise one configuration launch over all ends; an invalid
 *      end: INVALID_END.
 *   2. Attachments of an end x: the first `connections` by ascending (d2(Q[v], x), v) of the valid nodes v with
 *      d2 <= r2 (no lower bound).
 *   3. ONE edge launch covers every problem; per problem, in order: the direct edge QI -> QG, the start attachments
 *      QI -> Q[v] in rank order, the goal attachments Q[v] -> QG in rank order.  A valid direct edge: SOLVED, the
 *      path [QI, QG], cost = sqrt(d2(QI, QG)).
 *   4. Search.  init[v] = sqrt(d2) for the valid start attachments, +inf elsewhere; dist is the least fixed point of
 *      dist[v] = min(init[v], min over u in adj(v) of fl(dist[u] + w(u, v))).  Rounded addition is monotone and the
 *      weights are positive, so that fixed point is unique and is what Dijkstra's algorithm computes; the kernel
 *      relaxes in sweeps until one changes nothing, at most N of them.  Goal choice: among the valid goal
 *      attachments, rank j at node g_j, the least fl(dist[g_j] + sqrt(d2(Q[g_j], QG))), ties to the lowest rank;
 *      none finite: NO_PATH.  Walk back from the chosen node: at v stop if init[v] == dist[v], otherwise go to the
 *      lowest-index u in adj(v) with fl(dist[u] + w(u, v)) == dist[v]; dist strictly decreases (the lo2 rule), so
 *      the walk ends.  The path is QI, the nodes in travel order, QG, and cost the chosen total: the left-to-right
 *      sum of its segments.  A path of more than max_rows rows: LONG, n_out = 0.
 * MJPL_E_ARG: a NULL required pointer, connections outside 1..32, max_rows < 2, B < 0 (or above 2^24), N outside
 * 0..2^20, radius or step_dist <= 0, NaN or inf.  row_off, adj and w are not checked: they must be a build's.
 * B = 0 launches nothing.
 *
 * Options: "roadmap_chunk_bytes" (256 MiB: the edge batch of one launch of a build, and the distance workspace of
 * one search launch of a query whose graph does not fit in LDS) and "roadmap_lds_nodes" (the largest N whose
 * distances a query keeps in LDS) change launches and no bit of any output.  Read-only, of the last call:
 * "roadmap_last_edges" (build: candidate edges; query: edges validated), "roadmap_last_chunks" (build: edge
 * launches; query: search launches), "roadmap_last_sweeps" (query: relaxation sweeps summed over the problems that
 * searched; build: 0).  Both calls synchronise the engine's stream (the edge count comes back to the host) and
 * clear the edge pipeline's status word (mjpl_take_status). */
#define MJPL_ROADMAP_SOLVED      0
#define MJPL_ROADMAP_NO_PATH     1
#define MJPL_ROADMAP_NONFINITE   2
#define MJPL_ROADMAP_INVALID_END 3
#define MJPL_ROADMAP_LONG        4
typedef struct {
  double radius, step_dist;
  int32_t k, reserved;
} mjpl_roadmap_desc;
typedef struct {
  double radius, step_dist;
  int32_t connections, max_rows;
} mjpl_roadmap_query_desc;
int mjpl_roadmap_build(mjpl_engine *e, const mjpl_roadmap_desc *desc, const double *Q, int64_t N, uint8_t *node_valid,
                       int32_t *row_off, int32_t *adj, double *w);
int mjpl_roadmap_build_dev(mjpl_engine *e, const mjpl_roadmap_desc *desc, const double *dQ, int64_t N, uint8_t *dnode_valid,
                           int32_t *drow_off, int32_t *dadj, double *dw);
int mjpl_roadmap_query(mjpl_engine *e, const mjpl_roadmap_query_desc *desc, const double *Q, int64_t N,
                       const uint8_t *node_valid, const int32_t *row_off, const int32_t *adj, const double *w,
                       const double *QI, const double *QG, int64_t B, double *P, int32_t *n_out, int32_t *status,
                       double *cost);
int mjpl_roadmap_query_dev(mjpl_engine *e, const mjpl_roadmap_query_desc *desc, const double *dQ, int64_t N,
                           const uint8_t *dnode_valid, const int32_t *drow_off, const int32_t *dadj, const double *dw,
                           const double *dQI, const double *dQG, int64_t B, double *dP, int32_t *dn_out,
                           int32_t *dstatus, double *dcost);

/* ---- certified edge checks: no contact anywhere along an edge ------------------------------
 * mjpl_check_edges tests waypoints step_dist apart and nothing between them.  The calls below decide the
 * whole segment q(t) = QA + t (QB - QA), t in [0, 1], by free bubbles and adaptive bisection (DESIGN.md
 * section 5.11 has the proof).
 *
 * The lever table W[P][nplan] over the candidate pairs of mjpl_contact_pairs: one unit of planning
 * column c changes the distance of pair p by at most W[p][c].  It is made at mjpl_create and by
 * mjpl_set_planning without bounds, and again by mjpl_sweep_bounds or by a mjpl_sweep_edges* call whose
 * bounds differ from those in force.  A planning SLIDE joint needs finite bounds: without them every
 * hinge above it has lever +inf for the geoms below the slide.  mjpl_sweep_bounds(e, lo, hi): HOST arrays
 * of nplan bounds, either may be NULL (none); NaN and lo > hi are refused.  mjpl_sweep_levers computes the
 * table on the host only -- no device needed, like mjpl_program_dump: W receives P * nplan doubles if
 * cap >= P * nplan, and the call returns P (or a negative error).
 *
 * mjpl_sweep_measure: the bubble measurement at N rows.  HD[i][c] >= 0 (Q's layout): how far column c may
 * move from q_i; cap > 0.  With D_p = min(d_p, cap) and B_p = sum_c HD[i][c] W[p][c] (ascending c, terms
 * with W = 0 or HD = 0 skipped, inf stays inf):
 *   gap[i]   = min over non-allowed p of (D_p - margin_p), gap_pair[i] its lowest index: bit-identical
 *              to mjpl_clearance(q_i, distmax = cap);
 *   slack[i] = min over non-allowed p of (D_p - margin_p - B_p), slack_pair[i] its lowest index.
 * Without a non-allowed pair: cap and -1.  A non-finite row of Q: NaN and -1.  slack[i] > 0 means: no
 * configuration of the box |q_c - q_i,c| <= HD[i][c] is in contact (given that the box lies inside the
 * bounds in force).  HD itself is not checked: a negative or non-finite entry gives a meaningless slack.
 *
 * mjpl_sweep_edges: E edges.  Descriptor: d_min >= 0, the clearance every configuration of a FREE edge
 * keeps (0: no contact); cap > d_min + the largest margin of a non-allowed pair, where distances stop
 * being measured (and clear_lb saturates); max_depth 0..16 (8 is a good default); lo, hi as above.
 * A node (t, h) of an edge is the row q(t) with travel HD_c = h |QB_c - QA_c|.  Round 0 holds the end
 * points (0, 0), (1, 0) and the root (1/2, 1/2); depth k has h = 2^-(k+1).  Per node, on the outputs
 * of the measurement:
 *   hit        iff gap <= 0 or gap < d_min;
 *   certified  iff otherwise slack - d_min >= 1e-9;
 *   otherwise it is split into (t -+ h/2, h/2) -- or, at max_depth or for an end point, the edge is
 *   flagged undecided.
 * Rounds are breadth-first; an edge hit in a round opens no further nodes.
 *   status[i]   MJPL_SWEEP_HIT if any node hit, else UNDECIDED if flagged, else FREE: no configuration of
 *               the segment is in contact or nearer than d_min.  NONFINITE: the edge holds NaN / inf.
 *               RANGE: an end point lies outside the bounds given; the edge is not measured.
 *   t_hit[i]    the least t among the hit nodes of the first depth that has one; NaN unless HIT.
 *   pair[i]     that node's gap_pair; -1 unless HIT.
 *   clear_lb[i] the least certified slack over the edge's leaves: clearance(q(t)) >= clear_lb for all t,
 *               capped at cap; NaN unless FREE.
 *   depth[i], nodes[i]  the deepest depth evaluated and the number of nodes evaluated on the edge.
 * All outputs are deterministic.  MJPL_E_ARG: a parameter outside its range, NaN anywhere in the
 * descriptor, lo > hi, NULL descriptor, a NULL output with E > 0, an unknown layout.  MJPL_E_PAIRTYPE
 * as for mjpl_clearance.  The host forms synchronise; mjpl_sweep_edges_dev enqueues on the engine's
 * stream but synchronises it once per round to read how many nodes are open (4 bytes).  The results
 * depend on no option and no MJPL_* variable. */
#define MJPL_SWEEP_FREE       0
#define MJPL_SWEEP_HIT        1
#define MJPL_SWEEP_UNDECIDED  2
#define MJPL_SWEEP_NONFINITE  3
#define MJPL_SWEEP_RANGE      4
typedef struct {
  double d_min, cap;
  int32_t max_depth;
  const double *lo, *hi; /* host, [nplan], may be NULL, both forms */
} mjpl_sweep_desc;
int mjpl_sweep_levers(const mjpl_model_desc *model, const int32_t *allowed_bodies, int32_t nallowed,
                      const int32_t *qidx, int32_t nplan, const double *qpos_base, const double *lo,
                      const double *hi, double *W, int64_t cap);
int mjpl_sweep_bounds(mjpl_engine *e, const double *lo, const double *hi);
int mjpl_sweep_measure(mjpl_engine *e, const double *Q, const double *HD, int64_t N, int32_t layout, double cap,
                       double *slack, int32_t *slack_pair, double *gap, int32_t *gap_pair);
int mjpl_sweep_measure_dev(mjpl_engine *e, const double *dQ, const double *dHD, int64_t N, int32_t layout,
                           double cap, double *dslack, int32_t *dslack_pair, double *dgap, int32_t *dgap_pair);
int mjpl_sweep_edges(mjpl_engine *e, const mjpl_sweep_desc *desc, const double *QA, const double *QB, int64_t E,
                     int32_t layout, int32_t *status, double *t_hit, double *clear_lb, int32_t *pair,
                     int32_t *nodes, int32_t *depth);
int mjpl_sweep_edges_dev(mjpl_engine *e, const mjpl_sweep_desc *desc, const double *dQA, const double *dQB,
                         int64_t E, int32_t layout, int32_t *dstatus, double *dt_hit, double *dclear_lb,
                         int32_t *dpair, int32_t *dnodes, int32_t *ddepth);

/* ---- certified trajectories: no contact anywhere along the spline ----------------------------
 * mjpl_topp_* moves along the natural cubic spline through the waypoints, not along the polyline that
 * mjpl_sweep_edges certifies; the spline can leave the polyline, and the bounds, between its waypoints.
 * mjpl_sweep_splines decides the PIECES of B splines the way mjpl_sweep_edges decides edges (DESIGN.md
 * section 5.13; tests/spline_sweep_reference.py states every operation).
 *
 * W is packed [wp_off[B]][nplan] over the engine's planning columns and wp_off is a HOST array in both
 * forms, as for mjpl_topp_profile.  A path of n waypoints has n - 1 pieces; piece k of path b is
 *   q_k(B) = the spline on [k / (n-1), (k+1) / (n-1)] at the local coordinate B in [0, 1]
 * and its outputs sit at index wp_off[b] - b + k: wp_off[B] - B pieces in all.  M (may be NULL: not
 * wanted) receives the knot second derivatives, bit-identical to mjpl_topp_profile's M on the same W.
 *
 * A node (t, h) of a piece stands for B in [a, b] = [t - h, t + h].  Its row is q_k(t) -- for the end
 * points (0, 0) and (1, 0) the waypoint itself -- and its travel per column c, with r = n - 1 and q' the
 * derivative with respect to the path coordinate s:
 *   P0 = q_k(a), P3 = q_k(b), P1 = P0 + (b - a)/3 q_k'(a)/r, P2 = P3 - (b - a)/3 q_k'(b)/r,
 *   HD_c = max_j |P_j,c - row_c| (1 + 2^-30) + 2^-40 (|W_k,c| + |W_k+1,c| + (|M_k,c| + |M_k+1,c|) / (6 r^2)),
 * 0 when h = 0.  A cubic lies in the hull of its Bezier control points P0..P3, so every q_k(B) of the node
 * lies in the box row +- HD; the inflation covers the rounding of the control points.
 *
 * Rounds, depths, the measurement and the rule per node are those of mjpl_sweep_edges, with two
 * additions, tested in this order:
 *   a node whose ROW lies outside [lo, hi] in a column counts as a hit with pair -2, before contact is
 *     looked at: if it decides the piece, status is MJPL_SWEEP_RANGE, t_hit where it left, pair -2;
 *   a node whose BOX leaves [lo, hi] while its row does not is never certified (the lever table holds
 *     inside the bounds only): it is split -- or, at max_depth, the piece is undecided.  So a piece that
 *     touches a bound, at a waypoint or between two, is never FREE.
 * A piece with a waypoint outside the bounds is RANGE and is not measured (t_hit NaN, pair -1), as an
 * edge is.  A path with a non-finite waypoint has every piece NONFINITE (and a non-finite M); the other
 * paths of the batch are not affected.  status, t_hit (the local B), clear_lb, pair, nodes and depth per
 * piece are otherwise those of mjpl_sweep_edges, and FREE means: no configuration q_k(B), B in [0, 1], is
 * in contact or nearer than d_min, and clearance >= clear_lb all along the piece.
 * MJPL_E_ARG: what mjpl_sweep_edges refuses in the descriptor, a NULL W, wp_off or output with B > 0, a
 * path with fewer than 2 waypoints or offsets that fall, B < 0.  B = 0 launches nothing.  All outputs
 * are deterministic and depend on no option and no MJPL_* variable.  The host form synchronises; the
 * device form synchronises the engine's stream on entry (before the tables of an earlier call are
 * replaced) and once per round. */
int mjpl_sweep_splines(mjpl_engine *e, const mjpl_sweep_desc *desc, const double *W, const int64_t *wp_off, int64_t B,
                       double *M, int32_t *status, double *t_hit, double *clear_lb, int32_t *pair, int32_t *nodes,
                       int32_t *depth);
int mjpl_sweep_splines_dev(mjpl_engine *e, const mjpl_sweep_desc *desc, const double *dW, const int64_t *wp_off,
                           int64_t B, double *dM, int32_t *dstatus, double *dt_hit, double *dclear_lb, int32_t *dpair,
                           int32_t *dnodes, int32_t *ddepth);

/* ---- device-resident entry points (asynchronous on the engine's stream) --------- */

int mjpl_check_configs_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout,
                           uint8_t *dvalid);
int mjpl_check_edges_dev(mjpl_engine *e, const double *dQA, const double *dQB, int64_t E,
                         double step_dist, int32_t layout, int32_t flags, uint8_t *dvalid,
                         int32_t *dfirst_bad);
/* The device-pointer edge entry point cannot return MJPL_E_NONFINITE (it does not synchronise):
 * a NaN/inf or absurdly long edge gets valid = 0 and first_bad = -2, and a sticky status bit is
 * set on the device.  mjpl_take_status synchronises the engine's stream, stores MJPL_OK or
 * MJPL_E_NONFINITE (the status every mjpl_check_edges_dev call since the last take would have
 * returned) in *status and clears the bit.  The host-buffer mjpl_check_edges clears the bit
 * before it launches and reports it itself. */
int mjpl_take_status(mjpl_engine *e, int32_t *status);
/* as mjpl_check_configs_dev but one bit per configuration, packed by wavefront ballot:
 * bit (i & 63) of dbits[i >> 6]. */
int mjpl_check_configs_bits_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout,
                                uint64_t *dbits);

/* Brute-force nearest neighbour of each query among tree nodes (Tree.nearest_neighbor,
 * planning/tree.py:57-66): nodes SoA [nplan][cap] with n valid, queries SoA [nplan][M];
 * out_idx[j] = argmin_i ||node_i - query_j||, ties to the lowest index. */
int mjpl_nearest_dev(mjpl_engine *e, const double *dnodes, int64_t n, int64_t cap,
                     const double *dqueries, int64_t M, int32_t *dout_idx, double *dout_dist2);

/* The same over the node range [n0, n) only, behind an answer for the nodes below n0 (dprev_idx, dprev_dist2: what an
 * earlier mjpl_nearest_dev over the first n0 nodes returned for these queries; NULL, NULL: none): the result is the
 * whole scan's -- a node of the range wins only if it is strictly nearer, so ties still go to the lowest index
 * (Tree.nearest_neighbor, planning/tree.py:57-66, over a tree that has grown since it was last scanned). */
int mjpl_nearest_range_dev(mjpl_engine *e, const double *dnodes, int64_t n0, int64_t n, int64_t cap,
                           const double *dqueries, int64_t M, int32_t *dout_idx, double *dout_dist2,
                           const int32_t *dprev_idx, const double *dprev_dist2);

/* Which screen the last mjpl_nearest_dev ran in front of its float64 distances: 0 none (plain float64 scan),
 * 1 binary32 on the vector units, 2 binary16 operands on the matrix cores (large trees and query sets whose
 * coordinates are all below 256 in magnitude and whose nodes' squared norms are below 65504, the range of
 * binary16).  The result is the float64 scan's either way.  Synchronises. */
int32_t mjpl_nearest_last_screen(mjpl_engine *e);

/* ---- options: the switches tests and tools need, through the ABI instead of the caller's environment ----
 * mjpl_set_option(e, name, value): MJPL_OK, or MJPL_E_ARG for an unknown name / a value out of range.  Options
 * that shape the compiled model (e.g. "filter") take effect at the next mjpl_set_planning / first launch; the rest
 * at the next call.  Names: the table in tools/README.md ("nn_cells", "nn_cells_min_nodes", "nn_mfma",
 * "nn_sample", "filter", "fused", ...).  mjpl_get_option reads one back.  "prune_pairs" (default 1) shapes the compiled
 * model like "filter": the program leaves out every enabled pair proved never to pass its bounding cull -- 1: pairs of a
 * moving geom with a static geom or a plane, 2: pairs of two moving geoms of one chain as well, 0: none; the read-only
 * "pairs_pruned" holds how many.  "prune_contacts" (default 1; 0: off) likewise: pairs of a moving geom with a static geom
 * or a plane proved never to come within their margin are left out of a per-program library's generated check -- the
 * tables keep them, the program hash covers the set when it is not empty; read-only "pairs_never_touch",
 * "prune_contact_evals". */
int mjpl_set_option(mjpl_engine *e, const char *name, double value);
int mjpl_get_option(mjpl_engine *e, const char *name, double *value);
/* the table itself: how many options there are, and option `index`'s name (NULL beyond the table; *writable = 0 for a
 * read-only one).  The library reads NO switch from the environment -- except that with MJPL_DEBUG=1 set when an engine
 * is made, every writable option NAME is also taken from the variable MJPL_<NAME> (shell tools, A/B scripts). */
int32_t mjpl_option_count(void);
const char *mjpl_option_name(int32_t index, int32_t *writable);
/* per-model libraries (mjpl_amd/specialise.py) are looked for in `dir` instead of the directory `spec` beside this
 * library; NULL or "": the default again.  Process-wide; takes effect at the next mjpl_set_planning / mjpl_set_spec. */
int mjpl_set_spec_dir(const char *dir);

/* ---- device memory and stream helpers (so that hosts need no other GPU runtime) -- */

int mjpl_dev_alloc(mjpl_engine *e, size_t bytes, void **out);
int mjpl_dev_free(mjpl_engine *e, void *p);
int mjpl_h2d(mjpl_engine *e, void *dst, const void *src, size_t bytes);  /* async */
int mjpl_d2h(mjpl_engine *e, void *dst, const void *src, size_t bytes);  /* async */
int mjpl_sync(mjpl_engine *e);
/* raw hipStream_t of the engine, for interop with other runtimes */
void *mjpl_stream(mjpl_engine *e);

/* ---- measurement ---------------------------------------------------------------- */

/* Stages of one mjpl_check_edges* launch, in stream order.  With the float32 filter on:
 * endpoints of all edges (+ emission of the survivors' interior waypoints as work items), one lane
 * per waypoint item, the walking kernel for what was not expanded, the float64 re-check of the
 * undecided pairs / configurations, the float64 edge kernel for undecided whole edges.  With the
 * filter off the float64 edge kernel is the whole launch. */
#define MJPL_STAGE_ENDPOINTS 0  /* k_filter_endpoints (incl. the counter memset); with mjpl_info.fused_edges:
                                  * k_edges_fused, the whole float32 filter of the launch (stage 1 is then empty) */
#define MJPL_STAGE_ITEMS     1  /* k_filter_items                                          */
#define MJPL_STAGE_WALK      2  /* k_filter_edges                                          */
#define MJPL_STAGE_PATCH     3  /* k_patch_pairs (immediate interpreter: k_check_configs, patch mode); with mjpl_info.fused_tail:
                                  * k_tail, the one launch that holds the walking, pair and exact-edge roles (stages
                                  * 2 and 4 are then empty) */
#define MJPL_STAGE_EXACT     4  /* k_check_edges                                           */
#define MJPL_NSTAGES         5

/* Run mjpl_check_edges_dev `iters` times back to back on the engine's stream, timed with HIP
 * events recorded on that stream: two around the whole run (*ms_mean = mean duration of a call,
 * all kernels) and, on every `sample_every`-th call, one after each stage, so that
 * stage_ms[MJPL_NSTAGES] (nullable) receives each stage's mean duration over *nsamples (nullable)
 * sampled calls.  Sampling keeps the instrumentation below one percent of the run it measures;
 * sample_every > iters: no call is sampled (stage_ms untouched, *nsamples = 0).
 * Inputs and outputs are device-resident.  Used by bench.py for roofline.achieved. */
int mjpl_time_edges_stages_dev(mjpl_engine *e, const double *dQA, const double *dQB, int64_t E,
                               double step_dist, int32_t layout, uint8_t *dvalid, int32_t iters,
                               int32_t sample_every, float *ms_mean, float *stage_ms,
                               int32_t *nsamples);
/* The same with every call sampled: ms[k] = the mean call, ms_first[k] (nullable) = the mean
 * duration of the filter's item pass (filter off: of the float64 edge kernel). */
int mjpl_time_edges_dev(mjpl_engine *e, const double *dQA, const double *dQB, int64_t E,
                        double step_dist, int32_t layout, uint8_t *dvalid, int32_t iters,
                        float *ms, float *ms_first);
int mjpl_time_configs_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout,
                          uint8_t *dvalid, int32_t iters, float *ms);
/* iters times mjpl_topp_profile_dev then mjpl_topp_sample_dev on the same device batches, each between two
 * events: ms_profile[k], ms_sample[k] = what call k took on the stream, the upload of its offset tables
 * included.  samp_off must fit the durations the profile gives (size it from an earlier call). */
int mjpl_time_topp_dev(mjpl_engine *e, const mjpl_topp_desc *desc, const double *dW, const int64_t *wp_off, int64_t B,
                       double *dM, double *dx, double *du, double *dt_grid, int32_t *dstatus, double dt,
                       const int64_t *samp_off, double *dpos, double *dvel, double *dacc, int32_t iters,
                       float *ms_profile, float *ms_sample);
/* The same for mjpl_jerk_profile_dev and mjpl_jerk_sample_dev. */
int mjpl_time_jerk_dev(mjpl_engine *e, const mjpl_jerk_desc *desc, const double *dW, const int64_t *wp_off, int64_t B,
                       double *dM, double *dlim, double *dv, double *dvp, double *dtc, double *dt_grid, int32_t *dstatus,
                       double dt, const int64_t *samp_off, double *dpos, double *dvel, double *dacc, int32_t iters,
                       float *ms_profile, float *ms_sample);
/* iters times one sweep call between two events: with wp_off NULL mjpl_sweep_edges_dev(dA, dB, n edges, layout), else
 * mjpl_sweep_splines_dev(W = dA, wp_off, n paths, M = dB, which may be NULL); ms[k] = what call k took on the
 * stream, its table uploads and its per-round synchronisations included. */
int mjpl_time_sweep_dev(mjpl_engine *e, const mjpl_sweep_desc *desc, const double *dA, double *dB, const int64_t *wp_off,
                        int64_t n, int32_t layout, int32_t *dstatus, double *dt_hit, double *dclear_lb, int32_t *dpair,
                        int32_t *dnodes, int32_t *ddepth, int32_t iters, float *ms);

/* ---- misc ------------------------------------------------------------------------ */

int mjpl_device_count(void);
const char *mjpl_last_error(void);
const char *mjpl_version(void);

/* ---- PoseConstraint (src/mjpl/constraint/pose_constraint.py) ---
 * One handle per (engine, site, constraint frame).  Batches are rows of FULL qpos vectors,
 * [N][nq] (apply() receives and returns full configurations, pose_constraint.py:78-91). */
typedef struct mjpl_pose_desc {
  int32_t site_body;          /* model.site_bodyid[site] (pose_constraint.py:70)              */
  double  site_pos[3];        /* model.site_pos[site]                                          */
  double  site_quat[4];       /* model.site_quat[site], wxyz                                   */
  double  c_quat[4];          /* C_T_world = reference_frame.inverse() (:63): rotation, wxyz   */
  double  c_pos[3];           /*                                        translation           */
  double  lo[6], hi[6];       /* x y z roll pitch yaw bounds (:57-59)                          */
  double  tolerance;          /* :29 (>= 0)                                                    */
  double  q_step;             /* :30 (> 0; may be +inf)                                        */
  const double *jnt_range;    /* [njnt*2] JointLimitConstraint (joint_limit_constraint.py:16-17) */
  int32_t max_iters;          /* the reference loops without a bound (:80); <= 0 -> 1000       */
} mjpl_pose_desc;

typedef struct mjpl_pose mjpl_pose;

/* PoseConstraint.__init__ (pose_constraint.py:18-70); ValueError cases -> MJPL_E_ARG */
int mjpl_pose_create(mjpl_engine *e, const mjpl_pose_desc *desc, mjpl_pose **out);
/* 1: a generated projection of the engine's per-model library serves this handle (the chain from the world to the
 * site's body as straight-line code: mjpl_amd/specialise.py); 0: the interpreting kernels.
 * Same results either way, bit for bit.  MJPL_POSE_SPEC=0 at creation keeps a handle on the interpreting kernels. */
int mjpl_pose_spec_loaded(mjpl_pose *p);
/* Host only, no device needed: the chain program of (model, site body) that mjpl_pose_create compiles -- int words
 * [header | per chain body {njnt}, per joint {type, qadr, joint id}], doubles [per body pos[3] quat[4]; per joint
 * axis[3] pos[3] qpos0] -- and the hash a generated projection is looked up by.  pi = pd = NULL returns the sizes. */
int mjpl_pose_chain_dump(const mjpl_model_desc *model, int32_t site_body, int32_t *pi, int32_t *npi, double *pd, int32_t *npd,
                         uint64_t *hash);
void mjpl_pose_destroy(mjpl_pose *p);
/* `pose_constraint.q_step = ...` (examples/franka_constrained_move_to_pose.py:72-75) */
int mjpl_pose_set_q_step(mjpl_pose *p, double q_step);

/* Batched PoseConstraint.apply (pose_constraint.py:78-91): row i of Q is projected onto the
 * constraint starting from itself; ok[i] = 1 and Q_out row i = the projection, or ok[i] = 0
 * (the reference's None: joint limits violated or farther than 2*q_step from Q_old row i).
 * iters (nullable): projection steps taken; negative = gave up after max_iters (ok = 0). */
int mjpl_pose_apply(mjpl_pose *p, const double *Q_old, const double *Q, int64_t N, double *Q_out,
                    uint8_t *ok, int32_t *iters);
/* Batched PoseConstraint.valid_config (pose_constraint.py:72-76); xpos [N][3] / xmat [N][9]
 * (nullable) receive the site's world pose (utils.site_pose, src/mjpl/utils.py:60-75). */
int mjpl_pose_valid(mjpl_pose *p, const double *Q, int64_t N, uint8_t *valid, double *xpos, double *xmat);
/* device-pointer variants: asynchronous on the engine's stream */
int mjpl_pose_apply_dev(mjpl_pose *p, const double *dQ_old, const double *dQ, int64_t N, double *dQ_out,
                        uint8_t *dok, int32_t *diters);
int mjpl_pose_valid_dev(mjpl_pose *p, const double *dQ, int64_t N, uint8_t *dvalid, double *dxpos, double *dxmat);

/* ---- IK seeds (the role of MinkIKSolver.solve_ik,
 * src/mjpl/inverse_kinematics/mink_ik_solver.py:72-116).  The reference's arithmetic is a QP in
 * the un-vendored mink / daqp wheels; parity is tolerance-level (pose error within the
 * tolerances, constraints obeyed -- what test/test_mink_ik_solver.py:64-70 asserts).  Every row
 * of Q [N][nq] is one start configuration (q_init_guess or a random_config restart, :108-115)
 * iterated with damped least squares; joints with movable[j] == 0 are held (:63-70). */
typedef struct mjpl_ik_desc {
  int32_t site_body;          /* model.site_bodyid[site]                                       */
  double  site_pos[3];
  double  site_quat[4];       /* wxyz                                                          */
  double  target_pos[3];      /* pose: SE3 in the world frame (ik_solver_interface.py:13-19)   */
  double  target_quat[4];     /* wxyz                                                          */
  double  pos_tolerance;      /* mink_ik_solver.py:19 (metres)                                 */
  double  ori_tolerance;      /* :20 (radians)                                                 */
  int32_t iterations;         /* :23 iterations per attempt (>= 1)                             */
  double  damping;            /* Tikhonov term (reference: damping=1e-3 of the QP, :106); <= 0 -> 1e-6 */
  double  lm_damping;         /* error-proportional term (FrameTask lm_damping=0.1, :80); < 0 -> 0.1   */
  double  max_step;           /* |dq|_inf limit per iteration, radians / metres; <= 0 -> 0.2   */
  const double  *jnt_range;   /* [njnt*2] mink.ConfigurationLimit (:86)                        */
  const uint8_t *movable;     /* [njnt] 1 for the solver's `joints`, 0 for held joints         */
  int32_t restarts;           /* a stalled row re-draws its joints uniformly in their ranges, up to this
                               * many times within `iterations` (the reference restarts a failed attempt
                               * from random_config, :108-115); 0: none                           */
  uint64_t restart_seed;      /* seed of those draws                                           */
} mjpl_ik_desc;

/* ok[i] = 1 iff row i reached the target within the tolerances; Q_out row i is its final
 * iterate either way; iters (nullable) the iterations used; err (nullable) [N][2] the final
 * position / orientation error norms. */
int mjpl_ik_solve(mjpl_engine *e, const mjpl_ik_desc *desc, const double *Q, int64_t N, double *Q_out,
                  uint8_t *ok, int32_t *iters, double *err);
int mjpl_ik_solve_dev(mjpl_engine *e, const mjpl_ik_desc *desc, const double *dQ, int64_t N, double *dQ_out,
                      uint8_t *dok, int32_t *diters, double *derr);

/* ---- per-model specialised filter kernels ------------------------------
 * mjpl_create compiles a model into a program (control words + constant tables) that generic kernels
 * interpret.  mjpl_amd/specialise.py turns one such program into straight-line code, builds the
 * float32 filter kernels around it as libmjpl_spec_<hash>.so, and an engine whose program has that
 * hash launches them instead of the interpreting ones (same verdicts; MJPL_SPEC=0 disables,
 * MJPL_SPEC_DIR overrides the directory `spec` next to the library).  mjpl_program_dump compiles a
 * model on the host only -- no device needed -- and returns the program and its hash: call it with
 * ip = fp = dp = NULL for the sizes, then with buffers. */
typedef struct mjpl_program_info {
  uint64_t hash;            /* FNV-1a of (ip, fp, dp, kernel variant, MJPL_SPEC_ABI, digest of the shared headers) */
  int32_t maxs, wbox, mbox; /* kernel variant: slot-file width, static / moving boxes present */
  int32_t immediate;        /* 1: the model runs the immediate interpreter (more than 24 stored geoms: not specialisable) */
  int32_t filter_usable;
  float   filter_tol;
  int32_t nslots, nsave;
  int32_t spec_abi;
  /* scene-generic libraries (one per ROBOT: static geoms may change without a compiler): the hash of what
   * such a library carries as literals -- moving bodies, their geoms and self pairs, planning set,
   * tolerance -- the number of cull rows per moving geom it reads from the engine's scene table, and
   * whether this program can run on one (<= scene_rows static geoms, <= 24 moving geoms numbered
   * consecutively; not the immediate interpreter's programs) */
  uint64_t robot_hash;
  int32_t scene_rows;
  int32_t scene_ok;
} mjpl_program_info;
int mjpl_program_dump(const mjpl_model_desc *model, const int32_t *allowed_bodies, int32_t nallowed,
                      const int32_t *qidx, int32_t nplan, const double *qpos_base, double filter_tol,
                      int32_t *ip, int32_t *nip, float *fp, double *dp, int32_t *ntab,
                      mjpl_program_info *info);
/* The same with the option "prune_pairs" as an argument (0, 1 or 2; mjpl_program_dump: 1, the default of an engine) and the
 * pairs the program leaves out: *ndropped holds the room of `dropped` in pairs on entry (ignored when dropped is
 * NULL) and the number of dropped pairs on return; `dropped` receives (g1 < g2) geom ids, as many as fit.  These are
 * enabled pairs -- counted in mjpl_info.npairs -- proved never to come within their bounding radii and margin,
 * whatever the hinge angles; the candidate tables of mjpl_contacts*, mjpl_distances*,
 * mjpl_clearance* and mjpl_near_pairs* keep them. */
int mjpl_program_dump_pruned(const mjpl_model_desc *model, const int32_t *allowed_bodies, int32_t nallowed,
                             const int32_t *qidx, int32_t nplan, const double *qpos_base, double filter_tol,
                             int32_t prune_pairs, int32_t *ip, int32_t *nip, float *fp, double *dp, int32_t *ntab,
                             mjpl_program_info *info, int32_t *dropped, int32_t *ndropped);
/* The side set of the program compiled with the options "prune_pairs" and "prune_contacts" as given: the enabled pairs of
 * a moving geom with a static geom or a plane proved never to come within their contact margin, whatever the hinge angles
 * (DESIGN.md section 5.1d).  They stay in ip / fp / dp and in every table; a per-program library's generated check leaves
 * them out, and the program hash (*hash) covers the set when it is not empty.  *npairs: room of `pairs` in pairs on entry
 * (ignored when pairs is NULL), the size of the set on return; `pairs` receives (g1 < g2) geom ids, as many as fit;
 * *evals: cell evaluations the proofs took; *tables_hash: the hash of ip / fp / dp alone, which is the program hash of an
 * empty set.  prune_contacts: 0 the empty set, 1 an engine's default, >= 2 that many cell
 * evaluations per pair at most (tests). */
int mjpl_program_dump_never_touch(const mjpl_model_desc *model, const int32_t *allowed_bodies, int32_t nallowed,
                                  const int32_t *qidx, int32_t nplan, const double *qpos_base, double filter_tol,
                                  int32_t prune_pairs, int32_t prune_contacts, int32_t *pairs, int32_t *npairs,
                                  int32_t *evals, uint64_t *hash, uint64_t *tables_hash);
/* Host-only look-up, no device needed: is there a loadable library for this hash (mjpl_program_info.hash with
 * generic = 0, .robot_hash with generic = 1) that was built for this version of the engine?  1 / 0.  A
 * deployment step calls it after mjpl_amd/specialise.py; it is the look-up mjpl_create performs, and like it
 * may be called from any number of threads at once (the table of loaded libraries is the process's). */
int mjpl_spec_probe(uint64_t hash, int32_t generic);
/* 1 if the engine's current program runs on its own specialised library (hash of the whole program), 2 if
 * on the robot's scene-generic one (obstacles from a table), 0: the interpreting kernels */
int mjpl_spec_loaded(const mjpl_engine *e);
/* enable = 0: this engine runs the interpreting kernels whatever libraries exist (A/B measurements,
 * bench.py's "interpreter" variant); 1: look the libraries up again (the program's own first, then the
 * robot's scene-generic one); 2: the scene-generic one only (bench.py's "scene_generic" variant).
 * Synchronises. */
int mjpl_set_spec(mjpl_engine *e, int32_t enable);

/* ---- frontier bi-RRT, device-resident (BASELINE configs[3]) -------------
 * RRT.plan_to_configs' sample / extend / connect loop (src/mjpl/planning/rrt.py:190-235) for `lanes`
 * samples per round, with _constrained_extend's per-step rules (src/mjpl/planning/utils.py:139-164):
 * step <= epsilon towards the target, PoseConstraint projection first if a pose handle is given
 * (constraint order of examples/franka_constrained_move_to_pose.py:60-64), joint limits [lo, hi],
 * stop when a step moves less than 1e-8, leads away from the target, or fails the collision check
 * (endpoint + interval waypoints at interval_step; <= 0: endpoint only).  Both trees stay in HBM
 * as SoA slabs [nplan][capacity]; batches are over the engine's planning columns
 * (mjpl_set_planning).  The goal tree's roots are the goal configurations (the reference's sink
 * node, rrt.py:179-188, is implicit).  Rank k of W draws its own targets (counter-based generator
 * keyed by seed, k and the round); after every round all ranks' new nodes are all-gathered and
 * appended in rank order, so all ranks hold identical trees. */
typedef struct mjpl_rrt mjpl_rrt;

typedef struct mjpl_rrt_desc {
  int32_t lanes;               /* samples per rank per round                                   */
  int64_t capacity;            /* node capacity of each tree                                    */
  double  epsilon;             /* rrt.py:30                                                     */
  double  interval_step;       /* collision_interval_check step (rrt.py:28); <= 0: none         */
  double  goal_bias;           /* rrt.py:32                                                     */
  uint64_t seed;
  const double *lo, *hi;       /* [nplan] sampling box = JointLimitConstraint ranges            */
  mjpl_pose *pose;             /* nullable: PoseConstraint applied first                        */
  int64_t max_new_per_round;   /* slab rows per tree per rank per round; <= 0: max(128 lanes, 65536) */
  int32_t max_steps_per_round; /* most nodes a lane adds per extension; 0: no cap (the reference's
                                * _constrained_extend runs a chain to its end, planning/utils.py:139-164).
                                * > 0: a lane of the growing tree still under way after that many nodes is
                                * CARRIED -- it sits the connect phase out and, the next time its tree grows,
                                * goes on from the node it reached towards the same target instead of drawing
                                * a new one; a capped connect-phase lane just stops.  Deterministic per (lane,
                                * round): all ranks still hold identical trees. */
} mjpl_rrt_desc;

typedef struct mjpl_rrt_round_info {
  int32_t round;
  int32_t new_nodes[2];        /* appended this round, all ranks: start tree, goal tree         */
  int32_t nodes[2];            /* tree sizes after the round                                    */
  int32_t connected;           /* 1: a lane's two extensions met                                */
  int32_t conn_start, conn_goal; /* node ids of the junction in the start / goal tree           */
  int32_t conn_rank;           /* the rank whose lane connected (lowest rank, lowest lane wins) */
  int32_t stop_requested;      /* some rank passed request_stop != 0 this round                 */
} mjpl_rrt_round_info;

int mjpl_rrt_create(mjpl_engine *e, const mjpl_rrt_desc *desc, mjpl_rrt **out);
void mjpl_rrt_destroy(mjpl_rrt *r);
/* new query: start tree = {q_init}, goal tree = the ngoal rows of q_goals [ngoal][nplan] */
int mjpl_rrt_reset(mjpl_rrt *r, const double *q_init, const double *q_goals, int32_t ngoal, uint64_t seed);
/* one round: sample, extend the growing tree, extend the other towards what was reached, exchange.
 * Synchronises (the host needs the connection flag and the node counts).  request_stop != 0 (a
 * rank's time limit has passed) travels with the exchange, so that all ranks stop after the same
 * round: info->stop_requested.  An error that only one rank runs into (its slab of new nodes is
 * full, a HIP error) travels the same way: that rank still takes part in the exchange, and every
 * rank returns the error from the same round. */
int mjpl_rrt_round(mjpl_rrt *r, int32_t request_stop, mjpl_rrt_round_info *info);
/* The round split at its exchange step, for a launcher that moves the slabs itself (another
 * transport than RCCL; the tests, which run two ranks on one GPU): mjpl_rrt_round is
 *   round_begin -> all-gather of the headers -> all-gather of the slabs -> round_finish.
 * mjpl_rrt_set_world gives a planner its rank identity without a communicator (the sampler is keyed
 * by it, rrt.py:195-203 per rank); with mjpl_comm_init on the engine and no set_world the
 * communicator's rank / world are used.
 * round_begin: sample, extend, connect on this rank; synchronises; head[8] (host) receives this
 *   rank's exchange header: [0] new nodes of the tree that grew this round, [1] of the other tree,
 *   [2] connecting lane (INT32_MAX: none), [3] / [4] its node in the start / goal tree (>= 0: node id;
 *   < 0: -1 - index into this rank's slab), [5] stop request, [6] status of this rank's half
 *   (MJPL_OK, or the error every rank must return from round_finish), [7] 0.
 * round_slabs: device pointers of this rank's new nodes of pass p (0: the tree that grew, 1: the
 *   other): rows [head[p]][nplan] float64 and parents [head[p]] int32 (>= 0 node id, < 0 slab-relative).
 * round_finish: heads = all ranks' headers in rank order [world][8] (host); drows_all[p] /
 *   dparents_all[p] = device buffers holding every rank's slab of pass p, rank k at row offset
 *   k * stride_rows[p] (stride_rows[p] >= the largest head[p]; the pointers may be NULL when every
 *   count of the pass is 0).  Appends all slabs in rank order, resolves the winner (lowest rank),
 *   fills info.  The buffers must stay valid until the engine's stream has been synchronised. */
int mjpl_rrt_set_world(mjpl_rrt *r, int32_t rank, int32_t world);
int mjpl_rrt_round_begin(mjpl_rrt *r, int32_t request_stop, int32_t *head);
int mjpl_rrt_round_slabs(mjpl_rrt *r, int32_t pass, const void **drows, const void **dparents);
int mjpl_rrt_round_finish(mjpl_rrt *r, const int32_t *heads, const void *const *drows_all,
                          const void *const *dparents_all, const int32_t *stride_rows, mjpl_rrt_round_info *info);
/* after a round with connected = 1: the path q_init ... goal, rows [len][nplan] */
int mjpl_rrt_path(mjpl_rrt *r, double *path, int32_t maxlen, int32_t *len);
/* download a tree (0 = start, 1 = goal): rows Q [n][nplan] and parent ids (-1 = root); either may
 * be NULL; *n always receives the node count */
int mjpl_rrt_get_tree(mjpl_rrt *r, int32_t tree, double *Q, int32_t *parent, int64_t maxn, int64_t *n);
/* the targets [lanes][nplan] and participation flags of the most recent round (tests) */
int mjpl_rrt_get_lanes(mjpl_rrt *r, double *targets, uint8_t *on);

/* The exchange step runs on RCCL, called from this library on the engine's stream; a launcher only
 * ferries the 128-byte ncclUniqueId from rank 0 to the others (any transport).  Without a
 * communicator an engine is a world of one. */
int mjpl_comm_unique_id(void *id128);
int mjpl_comm_init(mjpl_engine *e, const void *id128, int32_t rank, int32_t world);
int mjpl_comm_destroy(mjpl_engine *e);
/* ncclAllGather of bytes_per_rank bytes per rank on the engine's stream (in place allowed:
 * dsend == drecv + rank * bytes_per_rank) */
int mjpl_allgather_dev(mjpl_engine *e, const void *dsend, void *drecv, size_t bytes_per_rank);

#ifdef __cplusplus
}
#endif
#endif
