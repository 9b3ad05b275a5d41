// mjpl_compile.h -- the model compiler of libmjpl_hip.so: host code only, no HIP call in this file.  Included by
// mjpl_hip.hip after mjpl_engine (same translation unit: HostModel, ModelLayout, FilterBound and fail are its).
// compile_host runs stages 1 to 6 (layout, ip / dp, error bound, float image, program hash, robot hash and scene
// table); load_spec and the upload follow in mjpl_hip.hip: compile_program.  Behind the stages: the host halves of the
// create-time tables and the chain program of the pose and IK handles.  No struct or table layout that crosses into a
// per-model library lives here (the stamped headers hold those).
#pragma once

namespace {

// FNV-1a, 64 bits: the program, robot and chain hashes
struct Fnv1a {
  uint64_t h = 0xcbf29ce484222325ull;
  void mix(const void *ptr, size_t n) {
    const unsigned char *b = (const unsigned char *)ptr;
    for (size_t k = 0; k < n; k++) { h ^= b[k]; h *= 0x100000001b3ull; }
  }
  void mixi(int v) { mix(&v, sizeof(v)); }
  void mixd(const double *v, int n) { mix(v, sizeof(double) * (size_t)n); }
  void mix_stamp() { const unsigned long long stamp = MJPL_SRC_STAMP; mix(&stamp, sizeof(stamp)); }  // the shared headers' digest
};

double norm3(const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

using BodyPairs = std::set<std::pair<int, int>>;  // sorted body-id pairs
using GeomPairs = std::set<std::pair<int, int>>;  // sorted geom-id pairs (g1 < g2)

bool pair_allowed(const HostModel &m, const BodyPairs &allowed, int g1, int g2) {
  const int b1 = m.geom_bodyid[g1], b2 = m.geom_bodyid[g2];
  return allowed.count({std::min(b1, b2), std::max(b1, b2)}) != 0;
}

// mj_collision's geometric pair filters [MJ-recalled: engine_collision_driver.c filterBitmask / filterBodyPair;
// oracle/mjpl_oracle.c: orc_collision's enumeration]: contype/conaffinity, same weld body, weld parent-child, and
// plane-plane, which has no collision function.  true: the pair is a candidate.
bool pair_candidate(const HostModel &m, int g1, int g2) {
  const int ct1 = m.geom_contype[g1], ca1 = m.geom_conaffinity[g1];
  const int ct2 = m.geom_contype[g2], ca2 = m.geom_conaffinity[g2];
  if (!(ct1 & ca2) && !(ct2 & ca1)) return false;
  const int w1 = m.body_weldid[m.geom_bodyid[g1]], w2 = m.body_weldid[m.geom_bodyid[g2]];
  if (w1 == w2) return false;
  const int wp1 = m.body_weldid[m.body_parentid[w1]];
  const int wp2 = m.body_weldid[m.body_parentid[w2]];
  if (w1 != 0 && w2 != 0 && (w1 == wp2 || w2 == wp1)) return false;
  return !(m.geom_type[g1] == GT_PLANE && m.geom_type[g2] == GT_PLANE);
}

// ... + the a6 ruleset folded in (CollisionRuleset: a contact between an allowed body pair never invalidates).
// true: the compiled program tests the pair.
bool pair_enabled(const HostModel &m, const BodyPairs &allowed, int g1, int g2) {
  return pair_candidate(m, g1, g2) && !pair_allowed(m, allowed, g1, g2);
}

bool type_supported(int t) { return t == GT_PLANE || t == GT_SPHERE || t == GT_CAPSULE || t == GT_BOX; }

// Cull bound and margin of the pair (g1 < g2, mj_collision's order): the squared sum of the bounding radii and the
// margin, or, beside a plane partner (`plane`: that geom, else -1), the other geom's radius and the margin as a
// distance; infinite where neither applies.
struct PairBound { double bound, margin; };
PairBound pair_bound(const HostModel &m, int g1, int g2, int plane) {
  PairBound pb;
  pb.margin = std::fmax(m.geom_margin[g1], m.geom_margin[g2]);
  const double r1 = m.geom_rbound[g1], r2 = m.geom_rbound[g2];
  pb.bound = std::numeric_limits<double>::infinity();
  if (r1 > 0 && r2 > 0) {
    const double bsum = r1 + r2 + pb.margin;
    pb.bound = bsum * bsum;
  } else if (plane >= 0) {
    const int other = plane == g1 ? g2 : g1;
    if (m.geom_rbound[other] > 0) pb.bound = pb.margin + m.geom_rbound[other];
  }
  return pb;
}

// ---- stage 1: the layout.  Validation failures in this order: joint types, welded bodies, unsupported geoms that a
// pair uses, capacity of the world tables, planes on moving bodies, register slots.
// static (world-welded) bodies and their geoms: poses folded here with the kernels' own arithmetic; the geoms take
// the rows of the world tables in geom-id order
int layout_statics(const HostModel &m, const BodyPairs &allowed, ModelLayout *L) {
  const int nb = m.nbody, ng = m.ngeom;
  L->body_static.assign(nb, 0);
  L->st_xpos.assign(3 * nb, 0.0);
  L->st_xquat.assign(4 * nb, 0.0);
  L->st_xmat.assign(9 * nb, 0.0);
  L->st_xquat[0] = 1.0;
  L->st_xmat[0] = L->st_xmat[4] = L->st_xmat[8] = 1.0;
  L->body_static[0] = 1;
  for (int b = 1; b < nb; b++) {
    if (m.body_weldid[b] != 0) continue;
    if (m.body_jntnum[b] != 0) return fail(MJPL_E_ARG, "body %d is welded to the world but has joints", b);
    const int p = m.body_parentid[b];
    if (!L->body_static[p]) return fail(MJPL_E_ARG, "body %d: weld id 0 below a moving parent", b);
    L->body_static[b] = 1;
    double np[3], nq[4];
    mul_mat_vec3(np, &L->st_xmat[9 * p], &m.body_pos[3 * b]);
    for (int k = 0; k < 3; k++) np[k] += L->st_xpos[3 * p + k];
    mul_quat(nq, &L->st_xquat[4 * p], &m.body_quat[4 * b]);
    normalize4(nq);
    for (int k = 0; k < 3; k++) L->st_xpos[3 * b + k] = np[k];
    for (int k = 0; k < 4; k++) L->st_xquat[4 * b + k] = nq[k];
    quat2mat(&L->st_xmat[9 * b], nq);
  }
  L->geom_static.assign(ng, 0);
  L->st_gxpos.assign(3 * ng, 0.0);
  L->st_gxmat.assign(9 * ng, 0.0);
  L->world_row.assign(ng, -1);
  for (int g = 0; g < ng; g++) {
    const int b = m.geom_bodyid[g];
    if (!type_supported(m.geom_type[g])) {
      // a geom that can never collide is harmless; otherwise refuse
      bool used = false;
      for (int h = 0; h < ng && !used; h++)
        if (h != g) used = pair_enabled(m, allowed, std::min(g, h), std::max(g, h));
      if (used) return fail(MJPL_E_PAIRTYPE, "geom %d has unsupported type %d", g, m.geom_type[g]);
    }
    if (!L->body_static[b]) { L->nmoving++; continue; }
    L->geom_static[g] = 1;
    double gp[3], gq[4];
    mul_mat_vec3(gp, &L->st_xmat[9 * b], &m.geom_pos[3 * g]);
    for (int k = 0; k < 3; k++) L->st_gxpos[3 * g + k] = gp[k] + L->st_xpos[3 * b + k];
    mul_quat(gq, &L->st_xquat[4 * b], &m.geom_quat[4 * g]);
    quat2mat(&L->st_gxmat[9 * g], gq);
    L->world_row[g] = (int)L->winfo.size();
    L->winfo.push_back(m.geom_type[g] | (g << 8));
    if (m.geom_type[g] == GT_PLANE) L->nplanes++;
  }
  if (L->nworld() > 64) return fail(MJPL_E_CAPACITY, "%d static geoms; this build enables at most 64 per moving geom", L->nworld());
  if (ng >= (1 << 23)) return fail(MJPL_E_CAPACITY, "too many geoms");
  return MJPL_OK;
}

// moving bodies in id order (parents precede children), where each takes its parent's pose from, LDS save slots;
// moving geoms in processing order, their partners, and register-slot allocation.  `dropped`: enabled pairs the program
// leaves out (prune_pairs, below): counted in npairs / npairs_world, on no partner list -- so slots, last_user, wbox /
// mbox and the per-geom masks follow the reduced lists
int layout_moving(const HostModel &m, const BodyPairs &allowed, const GeomPairs &dropped, ModelLayout *L) {
  const int ng = m.ngeom;
  for (int b = 1; b < m.nbody; b++)
    if (!L->body_static[b]) L->order.push_back(b);
  L->save_slot.assign(m.nbody, -1);
  L->parent_src.assign(L->order.size(), 0);
  for (size_t k = 0; k < L->order.size(); k++) {
    const int p = m.body_parentid[L->order[k]];
    if (L->body_static[p]) { L->parent_src[k] = PARENT_STATIC; continue; }
    if (k > 0 && L->order[k - 1] == p) { L->parent_src[k] = PARENT_CUR; continue; }
    if (L->save_slot[p] < 0) L->save_slot[p] = L->nsave++;
    L->parent_src[k] = L->save_slot[p] + 1;
  }
  L->stage_of.assign(ng, -1);
  for (int b : L->order)
    for (int g = 0; g < ng; g++)
      if (m.geom_bodyid[g] == b) { L->stage_of[g] = (int)L->mgeoms.size(); L->mgeoms.push_back(g); }
  const int nm = (int)L->mgeoms.size();
  L->stored_partners.assign(nm, {});
  L->world_partners.assign(nm, {});
  L->last_user.assign(nm, -1);
  auto note_pair = [&](int ga, int gb) {  // ga is the moving geom being placed
    if (m.geom_type[ga] == GT_BOX) L->mbox = true;
    if (m.geom_type[gb] == GT_BOX) (L->geom_static[gb] ? L->wbox : L->mbox) = true;
  };
  for (int k = 0; k < nm; k++) {
    const int g = L->mgeoms[k];
    for (int s = 0; s < ng; s++)
      if (L->geom_static[s] && pair_enabled(m, allowed, std::min(g, s), std::max(g, s))) {
        L->npairs++; L->npairs_world++;
        if (dropped.count({std::min(g, s), std::max(g, s)})) { L->npruned++; continue; }
        L->world_partners[k].push_back(s);
        note_pair(g, s);
      }
    for (int k2 = 0; k2 < k; k2++) {
      const int h = L->mgeoms[k2];
      if (!pair_enabled(m, allowed, std::min(g, h), std::max(g, h))) continue;
      L->npairs++;
      if (dropped.count({std::min(g, h), std::max(g, h)})) { L->npruned++; continue; }
      L->stored_partners[k].push_back(k2);
      note_pair(g, h);
      L->last_user[k2] = k;
    }
    if (m.geom_type[g] == GT_PLANE) return fail(MJPL_E_PAIRTYPE, "plane geom %d on a moving body", g);
  }
  // register slots: one per kept sphere/capsule, two per kept box; a slot is reusable once the
  // last geom that needs its occupant has been processed (a geom is stored after its own tests)
  L->slot_of.assign(nm, -1);
  std::vector<int> free_at;  // slot -> index of the last geom that reads it
  auto take = [&](int k) {
    for (size_t t = 0; t < free_at.size(); t++)
      if (free_at[t] <= k) { free_at[t] = L->last_user[k]; return (int)t; }
    free_at.push_back(L->last_user[k]);
    return (int)free_at.size() - 1;
  };
  for (int k = 0; k < nm; k++) {
    if (L->last_user[k] < 0) continue;
    const int s1 = take(k);
    const int s2 = (m.geom_type[L->mgeoms[k]] == GT_BOX) ? take(k) : (int)SLOT_NONE;
    L->slot_of[k] = s1 | (s2 << 6);
  }
  L->nslots = (int)free_at.size();
  if (L->nslots > MAX_SLOTS)
    return fail(MJPL_E_CAPACITY, "%d moving geoms must be held at once; this build has %d register slots",
                L->nslots, (int)MAX_SLOTS);
  L->maxs = L->nslots <= 4 ? 4 : (L->nslots <= 8 ? 8 : (L->nslots <= 16 ? 16 : 32));  // vector widths with indirect addressing
  return MJPL_OK;
}

int layout_model(const HostModel &m, const BodyPairs &allowed, const GeomPairs &dropped, const std::vector<int> &qidx,
                 ModelLayout *L) {
  *L = ModelLayout();
  for (int j = 0; j < m.njnt; j++)
    if (m.jnt_type[j] != JT_SLIDE && m.jnt_type[j] != JT_HINGE)
      return fail(MJPL_E_JOINT, "joint %d has type %d; only slide(2)/hinge(3) are supported", j,
                  m.jnt_type[j]);
  MJPL_TRY(layout_statics(m, allowed, L));
  MJPL_TRY(layout_moving(m, allowed, dropped, L));
  L->col_of.assign(m.nq, -1);
  for (int c = 0; c < (int)qidx.size(); c++) L->col_of[qidx[c]] = c;
  return MJPL_OK;
}

// ---- stage 1b: enabled pairs whose bounding cull can never pass.  A pair is dropped only on a
// PROOF over every hinge angle -- planned or not, so neither the planning selection nor the base configuration enters:
//   the moving geom's centre c lies within rad_k of O_k, the origin of chain body k before its own joints, where
//   rad_k = the body offsets, twice the joint offsets and the geom offset behind O_k (the ball of scene_table's
//   `breach`, taken from every ancestor instead of the world origin alone); O_k depends on the hinges in front of it;
//   with none O_k is a fixed point; with up to kPruneMaxHinges the hinge cube [-pi, pi]^h is bisected: in a cell of
//   half widths w_i around a centre angle vector, O_k is within sum_i w_i lever_i of its place at the centre (a rotation
//   by d about an axis moves a point at most d times its distance from a point of the axis, and lever_i bounds the
//   distance of O_k from hinge i's anchor in every configuration).
// Dropped when, for some k, in every cell:  |O_k - X| - rad_k - r1 - r2 - margin > kPruneSlack + widen (a plane: the
// signed height of O_k instead of |O_k - X|), X = the partner's centre: a static geom in the world frame, or an earlier
// moving geom of the same chain in its own body's frame (only the joints between the two count).  `widen` is what the
// binary32 culls add to the float64 threshold (float_image, scene_table).  Slide joints on the chain, infinite bounds,
// partners on another branch, more hinges than kPruneMaxHinges in front of every useful O_k, or a spent budget: kept.
constexpr double kPruneSlack = 1e-3;        // metres of proved clearance beyond every cull threshold
constexpr int kPruneMaxHinges = 3;          // hinges the bisection covers
constexpr int kPrunePairEvals = 8192;       // cell evaluations one pair may spend ...
constexpr int kPruneModelEvals = 1 << 18;  // ... and all pairs of a model together: the hard budget of a compile, once for
                                           // the pairs with static geoms and once for the self pairs

struct PruneChain {
  double bpos[3] = {0, 0, 0}, bquat[4] = {1, 0, 0, 0};  // the frame the chain hangs in
  std::vector<int> bodies;                               // from that frame down to the moving geom's body
  double base_reach = 0;                                 // |bpos|
};

// forward kinematics of bodies[0 .. k) at hinge angles th (in chain order), then the offset `off` in the last frame;
// line: per hinge its anchor and unit axis in the chain's frame
void prune_point(const HostModel &m, const PruneChain &c, int k, const double *th, const double *off, double *out,
                 double *line, double *quat_out = nullptr) {
  double pos[3] = {c.bpos[0], c.bpos[1], c.bpos[2]}, quat[4] = {c.bquat[0], c.bquat[1], c.bquat[2], c.bquat[3]};
  int h = 0;
  for (int i = 0; i < k; i++) {
    const int b = c.bodies[i];
    double d[3], q[4];
    rot_vec_quat(d, &m.body_pos[3 * b], quat);
    for (int a = 0; a < 3; a++) pos[a] += d[a];
    mul_quat(q, quat, &m.body_quat[4 * b]);
    normalize4(q);
    for (int a = 0; a < 4; a++) quat[a] = q[a];
    for (int j = 0; j < m.body_jntnum[b]; j++, h++) {
      const int jid = m.body_jntadr[b] + j;
      const double *ax = &m.jnt_axis[3 * jid], n = norm3(ax), inv = 1.0 / (n > 0 ? n : 1.0), s = std::sin(0.5 * th[h]) * inv;
      const double jq[4] = {std::cos(0.5 * th[h]), s * ax[0], s * ax[1], s * ax[2]};
      double anchor[3], back[3], axw[3];
      rot_vec_quat(anchor, &m.jnt_pos[3 * jid], quat);
      rot_vec_quat(axw, ax, quat);
      for (int a = 0; a < 3; a++) { line[6 * h + a] = pos[a] + anchor[a]; line[6 * h + 3 + a] = axw[a] * inv; }
      mul_quat(q, quat, jq);
      normalize4(q);
      for (int a = 0; a < 4; a++) quat[a] = q[a];
      rot_vec_quat(back, &m.jnt_pos[3 * jid], quat);
      for (int a = 0; a < 3; a++) pos[a] += anchor[a] - back[a];
    }
  }
  rot_vec_quat(out, off, quat);
  for (int a = 0; a < 3; a++) out[a] += pos[a];
  if (quat_out)  // (the last frame's orientation: stage 1c places a whole geom with it)
    for (int a = 0; a < 4; a++) quat_out[a] = quat[a];
}

// twice the joint offsets of body b from its joint `from` on
double prune_jlen(const HostModel &m, int b, int from) {
  double s = 0;
  for (int j = from; j < m.body_jntnum[b]; j++) s += 2.0 * norm3(&m.jnt_pos[3 * (m.body_jntadr[b] + j)]);
  return s;
}

// lever[h]: how far a point at most `tail` from the origin of chain body k's frame (before its joints; k = n: the last
// body's frame) can be from the anchor of hinge h, a hinge of bodies[0 .. k), in every configuration
void prune_levers(const HostModel &m, const PruneChain &c, int k, double tail, double *lever) {
  for (int i = 0, h = 0; i < k; i++)
    for (int j = 0; j < m.body_jntnum[c.bodies[i]]; j++, h++) {
      double l = norm3(&m.jnt_pos[3 * (m.body_jntadr[c.bodies[i]] + j)]) + prune_jlen(m, c.bodies[i], j + 1);
      for (int t = i + 1; t < k; t++) l += norm3(&m.body_pos[3 * c.bodies[t]]) + prune_jlen(m, c.bodies[t], 0);
      lever[h] = l + tail;
    }
}

// The worst-first bisection of the hinge cube [-pi, pi]^nh, shared by stages 1b and 1c.  bound_cell(cell) sets cell.low, a
// lower bound of the gap over the cell, and cell.widest, the hinge to split next; it returns false when the cell's centre
// itself is within the bound (no finer cell helps).  1: the worst cell left is clear -- proved; 0: a centre refused;
// -1: the pair's budget or the model's is spent (*pair_evals and *evals count the cell evaluations).
struct PruneCell {
  double th[kPruneMaxHinges], w[kPruneMaxHinges], low;
  int widest;
  bool operator<(const PruneCell &o) const { return low > o.low; }
};
template <class BoundCell>
int prune_bisect(int nh, int *pair_evals, int pair_budget, int *evals, int model_budget, BoundCell &&bound_cell) {
  std::priority_queue<PruneCell> todo;
  PruneCell root;
  for (int h = 0; h < kPruneMaxHinges; h++) { root.th[h] = 0.0; root.w[h] = h < nh ? 3.14159265358979323846 : 0.0; }
  if (++*pair_evals > pair_budget || ++*evals > model_budget) return -1;
  bool ok = bound_cell(root);
  todo.push(root);
  while (ok && todo.top().low <= 0) {
    const PruneCell cell = todo.top();
    todo.pop();
    if ((*pair_evals += 2) > pair_budget || (*evals += 2) > model_budget) return -1;
    PruneCell lo = cell, hi = cell;
    lo.w[cell.widest] = hi.w[cell.widest] = 0.5 * cell.w[cell.widest];
    lo.th[cell.widest] -= lo.w[cell.widest];
    hi.th[cell.widest] += hi.w[cell.widest];
    ok = bound_cell(lo) && bound_cell(hi);
    todo.push(lo);
    todo.push(hi);
  }
  return ok ? 1 : 0;
}

// true: proved.  X: the partner's centre in the chain's frame; nrm: a plane partner's normal (else nullptr); rsum: bounding
// radii and margin; need: kPruneSlack + widen; *evals: the model's counter.  Cells are split worst first (the one
// whose bound on the gap is lowest), so a pair that does come within reach is given up at the first cell centre that
// shows it, and a proof ends when the worst cell left is clear.
bool prune_prove(const HostModel &m, const PruneChain &c, int g, const double *X, const double *nrm, double rsum, double need,
                 int *evals) {
  const int n = (int)c.bodies.size();
  int pair_evals = 0;
  // k = n: the geom's centre itself (rad 0)
  for (int k = 0, nh = 0; k <= n; nh += k < n ? m.body_jntnum[c.bodies[k]] : 0, k++) {
    if (nh > kPruneMaxHinges) break;
    const double *off = k < n ? &m.body_pos[3 * c.bodies[k]] : &m.geom_pos[3 * g];
    double rad = 0;
    if (k < n) {
      rad = norm3(&m.geom_pos[3 * g]);
      for (int i = k; i < n; i++) rad += prune_jlen(m, c.bodies[i], 0) + (i > k ? norm3(&m.body_pos[3 * c.bodies[i]]) : 0.0);
    }
    double lever[kPruneMaxHinges] = {0, 0, 0};  // O_k from hinge i's anchor, at most, in every configuration
    prune_levers(m, c, k, norm3(off), lever);
    // false: the pair comes within reach at the cell's centre (no finer cell proves this k)
    auto bound_cell = [&](PruneCell &cell) {
      double O[3], line[6 * kPruneMaxHinges];
      prune_point(m, c, k, cell.th, off, O, line);
      const double d[3] = {O[0] - X[0], O[1] - X[1], O[2] - X[2]};
      const double gap = (nrm ? nrm[0] * d[0] + nrm[1] * d[1] + nrm[2] * d[2] : norm3(d)) - rad - rsum - need;
      // hinge i moves O_k by at most w_i times its distance from the axis: that distance at the centre plus what the
      // hinges behind i can add to it inside the cell, and never more than the lever
      double sway = 0, behind = 0, most = -1.0;
      cell.widest = 0;
      for (int h = nh - 1; h >= 0; h--) {
        const double *a = &line[6 * h], r[3] = {O[0] - a[0], O[1] - a[1], O[2] - a[2]};
        const double x[3] = {r[1] * a[5] - r[2] * a[4], r[2] * a[3] - r[0] * a[5], r[0] * a[4] - r[1] * a[3]};
        const double arm = std::fmin(lever[h], norm3(x) + behind), part = cell.w[h] * arm;
        sway += part;
        behind += cell.w[h] * lever[h];
        if (part > most) { most = part; cell.widest = h; }
      }
      cell.low = gap - sway;
      return gap > 0;
    };
    const int res = prune_bisect(nh, &pair_evals, kPrunePairEvals, evals, kPruneModelEvals, bound_cell);
    if (res != 0) return res > 0;  // (proved, or a budget spent; a centre within reach: the next k)
  }
  return false;
}

// the chain from `top` (exclusive: a static body, or the earlier geom's body) down to body b; false: b does not hang
// below `top`, or a slide joint lies between
bool prune_chain(const HostModel &m, const ModelLayout &L, int b, int top, PruneChain *c) {
  c->bodies.clear();
  for (int x = b; x != top; x = m.body_parentid[x]) {
    if (x == 0 || L.body_static[x]) {
      if (top >= 0) return false;
      break;
    }
    for (int j = 0; j < m.body_jntnum[x]; j++)
      if (m.jnt_type[m.body_jntadr[x] + j] != JT_HINGE) return false;
    c->bodies.push_back(x);
  }
  if (c->bodies.empty()) return false;
  std::reverse(c->bodies.begin(), c->bodies.end());
  if (top < 0) {
    const int p = m.body_parentid[c->bodies[0]];
    for (int a = 0; a < 3; a++) c->bpos[a] = L.st_xpos[3 * p + a];
    for (int a = 0; a < 4; a++) c->bquat[a] = L.st_xquat[4 * p + a];
  }
  c->base_reach = norm3(c->bpos);
  return true;
}

// L: the layout with every enabled pair on its lists; tol, poison_slack: the band and the widening float_image applies
// (upper bounds of what the reduced program will use); self_pairs: pairs of two moving geoms as well (option "prune_pairs"
// = 2).  Returns the cell evaluations spent.
int prune_pairs(const HostModel &m, const ModelLayout &L, double tol, double poison_slack, bool self_pairs,
                GeomPairs *dropped) {
  dropped->clear();
  const int nm = (int)L.mgeoms.size();
  const double u24 = std::ldexp(1.0, -24);
  // (two counters, each with the model's budget: what the scene costs must not change which SELF pairs are proved -- the
  //  robot hash of a scene-generic library covers them)
  int evals = 0, self_evals = 0;
  for (int k = 0; k < nm; k++) {
    const int g = L.mgeoms[k], b = m.geom_bodyid[g];
    // what the binary32 culls add to the float64 threshold thr of a partner at distance nx from the frame's origin:
    // the band and the pose error (at most half of it) of float_image, the form's allowance of scene_table /
    // expanded_threshold in squared distances (sqrt(thr^2 + a) <= thr + a / (2 thr)), the rounding of the thresholds
    auto widen = [&](const PruneChain &c, double nx, double thr, bool plane) {
      double reach = c.base_reach + norm3(&m.geom_pos[3 * g]);
      for (int x : c.bodies) {
        reach += norm3(&m.body_pos[3 * x]);
        for (int j = 0; j < m.body_jntnum[x]; j++) reach += 2.0 * norm3(&m.jnt_pos[3 * (m.body_jntadr[x] + j)]);
      }
      const double s = 1.01 * reach + nx;
      // (8 u s^2 is the allowance the threshold is raised by; the computed |c|^2 + a . c may fall short of the real value
      //  by up to 6 u s^2 more -- three squares, three products, their sums: 14 u s^2 in all)
      const double form = plane ? 4.0 * u24 * (s + thr) : 14.0 * u24 * s * s / (2.0 * thr);
      return 2.0 * tol + poison_slack + form + 1e-5 * (thr + s);
    };
    PruneChain c;
    if (!prune_chain(m, L, b, -1, &c)) continue;  // (a slide joint above the geom: unbounded reach, every pair kept)
    {
      for (int sgeom : L.world_partners[k]) {
        const bool plane = m.geom_type[sgeom] == GT_PLANE;
        const PairBound pb = pair_bound(m, std::min(g, sgeom), std::max(g, sgeom), plane ? sgeom : -1);
        if (!std::isfinite(pb.bound)) continue;
        const double rsum = plane ? pb.bound : std::sqrt(pb.bound);  // (radii and margin)
        if (!(rsum > 0)) continue;
        const double *X = &L.st_gxpos[3 * sgeom], *gm = &L.st_gxmat[9 * sgeom];
        const double nrm[3] = {gm[2], gm[5], gm[8]};
        if (prune_prove(m, c, g, X, plane ? nrm : nullptr, rsum, kPruneSlack + widen(c, norm3(X), rsum, plane), &evals))
          dropped->insert({std::min(g, sgeom), std::max(g, sgeom)});
      }
    }
    if (!self_pairs) continue;
    for (int k2 : L.stored_partners[k]) {
      const int h = L.mgeoms[k2];
      const PairBound pb = pair_bound(m, std::min(g, h), std::max(g, h), -1);
      if (!std::isfinite(pb.bound) || !(pb.bound > 0)) continue;
      PruneChain cm;  // (the frame of h's body: identity)
      if (!prune_chain(m, L, b, m.geom_bodyid[h], &cm)) continue;
      // (the kernels compare the two centres in the world frame: the form's rounding is that of the world chain's reach)
      const double rsum = std::sqrt(pb.bound);
      if (prune_prove(m, cm, g, &m.geom_pos[3 * h], nullptr, rsum, kPruneSlack + widen(c, 0.0, rsum, false), &self_evals))
        dropped->insert({std::min(g, h), std::max(g, h)});
    }
  }
  return std::min(evals, kPruneModelEvals) + std::min(self_evals, kPruneModelEvals);  // cell evaluations spent
}

// ---- stage 1c: enabled pairs of a moving geom with a static geom or plane that pass their bounding cull somewhere but
// can never come within their contact margin.  The same domain, chain, forward kinematics and
// worst-first bisection as stage 1b; what differs:
//   the gap at a cell's centre is the float64 distance between the two CORES (sphere: a point, capsule: a segment, box:
//   the solid box, plane: the half space) minus both radii and the margin, the moving geom placed with ALL hinges above
//   it (the ball around an ancestor's origin says nothing about where a capsule's ends are);
//   inside a cell hinge i moves any point of the moving core by at most w_i times that point's distance from the axis.
//   The distance from a line is convex, so over a core it is largest at one of the core's extreme points (the point, the
//   segment's two ends, the box's eight corners): arm_i = the largest of them at the cell's centre plus what the hinges
//   behind i add inside the cell, and never more than lever_i + the core's half extent (half length, half diagonal, 0).
// A pair is proved when in every cell  gap - sum_i w_i arm_i > slack,  slack = kPruneSlack + 2 tol + the poison widening:
// the filter classifies a pair by ITS distance against margin +- tol (classify), and that distance is within the band tol
// of the float64 one (filter_error_bound: that is what the band is), so a real gap above 2 tol is called neither contact
// nor unsure -- and a routine that is more cautious than that only hands the pair to the exact re-check, which clears it:
// verdicts never depend on the set.  kPruneSlack (1 mm) is far above the float64 rounding of the routines below and the
// 1e-9 the segment-box minimisation stops at.  A poisoned static partner (NaN rows: always unsure), box against box, a
// slide joint on the chain, an infinite size, more than kPruneMaxHinges hinges above the geom, a spent budget: kept.
// The proved pairs stay in ip / fp / dp, the masks and every table: only a per-program generated check leaves them out.
constexpr int kContactPairEvals = 8192;      // cell evaluations one pair may spend (option "prune_contacts" >= 2: that many) ...
constexpr int kContactModelEvals = 1 << 18;  // ... and all pairs of a model together

struct PruneCore {
  int type = GT_SPHERE;
  double c[3] = {0, 0, 0}, R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, size[3] = {0, 0, 0};  // R: row-major, its columns the axes
  double radius() const { return type == GT_SPHERE || type == GT_CAPSULE ? size[0] : 0.0; }
  double half_extent() const { return type == GT_CAPSULE ? size[1] : (type == GT_BOX ? norm3(size) : 0.0); }
  // the extreme points of the core: 1, 2 or 8 (a plane: none)
  int points(double (*p)[3]) const {
    if (type == GT_SPHERE) { for (int a = 0; a < 3; a++) p[0][a] = c[a]; return 1; }
    if (type == GT_CAPSULE) {
      for (int a = 0; a < 3; a++) { p[0][a] = c[a] - size[1] * R[3 * a + 2]; p[1][a] = c[a] + size[1] * R[3 * a + 2]; }
      return 2;
    }
    if (type != GT_BOX) return 0;
    for (int k = 0; k < 8; k++)
      for (int a = 0; a < 3; a++)
        p[k][a] = c[a] + (k & 1 ? 1 : -1) * size[0] * R[3 * a] + (k & 2 ? 1 : -1) * size[1] * R[3 * a + 1] +
                  (k & 4 ? 1 : -1) * size[2] * R[3 * a + 2];
    return 8;
  }
};

double dist_point_point(const double *p, const double *q) {
  const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  return norm3(d);
}

double dist_point_segment(const double *p, const double *a, const double *b) {
  const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const double len2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
  double t = len2 > 0 ? (ap[0] * ab[0] + ap[1] * ab[1] + ap[2] * ab[2]) / len2 : 0.0;
  t = std::fmin(1.0, std::fmax(0.0, t));
  const double q[3] = {a[0] + t * ab[0], a[1] + t * ab[1], a[2] + t * ab[2]};
  return dist_point_point(p, q);
}

// closest points of two segments, clamped; near-parallel segments leave the parameter of the first ill-conditioned, so
// the four end-against-segment distances (exact in that case) are taken in as well
double dist_segment_segment(const double *a0, const double *a1, const double *b0, const double *b1) {
  const double d1[3] = {a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]}, d2[3] = {b1[0] - b0[0], b1[1] - b0[1], b1[2] - b0[2]};
  const double r[3] = {a0[0] - b0[0], a0[1] - b0[1], a0[2] - b0[2]};
  auto dot = [](const double *x, const double *y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; };
  auto clamp01 = [](double v) { return std::fmin(1.0, std::fmax(0.0, v)); };
  const double a = dot(d1, d1), e = dot(d2, d2), f = dot(d2, r), c = dot(d1, r), b = dot(d1, d2);
  double best = std::fmin(std::fmin(dist_point_segment(a0, b0, b1), dist_point_segment(a1, b0, b1)),
                          std::fmin(dist_point_segment(b0, a0, a1), dist_point_segment(b1, a0, a1)));
  const double denom = a * e - b * b;
  if (a > 0 && e > 0 && denom > 0) {
    double s = clamp01((b * f - c * e) / denom), t = (b * s + f) / e;
    if (t < 0) { t = 0; s = clamp01(-c / a); }
    else if (t > 1) { t = 1; s = clamp01((b - c) / a); }
    const double p[3] = {a0[0] + s * d1[0], a0[1] + s * d1[1], a0[2] + s * d1[2]};
    const double q[3] = {b0[0] + t * d2[0], b0[1] + t * d2[1], b0[2] + t * d2[2]};
    best = std::fmin(best, dist_point_point(p, q));
  }
  return best;
}

double dist_point_box(const double *p, const PruneCore &box) {
  const double d[3] = {p[0] - box.c[0], p[1] - box.c[1], p[2] - box.c[2]};
  double out2 = 0;
  for (int k = 0; k < 3; k++) {
    const double x = std::fabs(d[0] * box.R[k] + d[1] * box.R[3 + k] + d[2] * box.R[6 + k]) - box.size[k];
    if (x > 0) out2 += x * x;
  }
  return std::sqrt(out2);
}

// the distance of the segment's point at t from the box is convex in t: a ternary search to 1e-9 of the segment's length
double dist_segment_box(const double *a, const double *b, const PruneCore &box) {
  auto at = [&](double t) {
    const double p[3] = {a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), a[2] + t * (b[2] - a[2])};
    return dist_point_box(p, box);
  };
  double lo = 0.0, hi = 1.0;
  for (int it = 0; it < 52; it++) {  // ((2/3)^52 < 1e-9)
    const double m1 = lo + (hi - lo) / 3.0, m2 = hi - (hi - lo) / 3.0;
    if (at(m1) <= at(m2)) hi = m2; else lo = m1;
  }
  return std::fmin(at(0.5 * (lo + hi)), std::fmin(at(0.0), at(1.0)));
}

// distance between the cores of a moving geom A and a static geom or plane S; NaN: no routine (box against box)
double core_distance(const PruneCore &A, const PruneCore &S) {
  double pa[8][3], ps[8][3];
  const int na = A.points(pa);
  if (S.type == GT_PLANE) {  // the lowest extreme point above the plane (negative: below it)
    double low = std::numeric_limits<double>::infinity();
    for (int k = 0; k < na; k++) {
      double h = 0;
      for (int a = 0; a < 3; a++) h += S.R[3 * a + 2] * (pa[k][a] - S.c[a]);
      low = std::fmin(low, h);
    }
    return na ? low : std::numeric_limits<double>::quiet_NaN();
  }
  const int ns = S.points(ps);
  if (na == 0 || ns == 0 || (na == 8 && ns == 8)) return std::numeric_limits<double>::quiet_NaN();
  if (na == 8) return ns == 1 ? dist_point_box(ps[0], A) : dist_segment_box(ps[0], ps[1], A);
  if (ns == 8) return na == 1 ? dist_point_box(pa[0], S) : dist_segment_box(pa[0], pa[1], S);
  if (na == 1 && ns == 1) return dist_point_point(pa[0], ps[0]);
  if (na == 1) return dist_point_segment(pa[0], ps[0], ps[1]);
  if (ns == 1) return dist_point_segment(ps[0], pa[0], pa[1]);
  return dist_segment_segment(pa[0], pa[1], ps[0], ps[1]);
}

// true: proved.  c: the chain from the world down to geom g's body; S: the partner in the world frame; rsum: both radii
// and the margin; need: the slack; budget: cell evaluations this pair may spend; *evals: the model's counter.
bool contact_prove(const HostModel &m, const PruneChain &c, int g, const PruneCore &S, double rsum, double need, int budget,
                   int *evals) {
  const int n = (int)c.bodies.size();
  int nh = 0;
  for (int b : c.bodies) nh += m.body_jntnum[b];
  if (nh > kPruneMaxHinges) return false;
  PruneCore A;
  A.type = m.geom_type[g];
  for (int a = 0; a < 3; a++) A.size[a] = m.geom_size[3 * g + a];
  const double ext = A.half_extent();
  double lever[kPruneMaxHinges] = {0, 0, 0};  // any point of the core from hinge i's anchor, at most, in every configuration
  prune_levers(m, c, n, norm3(&m.geom_pos[3 * g]) + ext, lever);
  // false: within the slack of contact at the cell's centre (or no routine for the pair)
  auto bound_cell = [&](PruneCell &cell) {
    double line[6 * kPruneMaxHinges], bq[4], gq[4], pts[8][3];
    prune_point(m, c, n, cell.th, &m.geom_pos[3 * g], A.c, line, bq);
    mul_quat(gq, bq, &m.geom_quat[4 * g]);
    normalize4(gq);
    quat2mat(A.R, gq);
    const double gap = core_distance(A, S) - rsum - need;
    const int np = A.points(pts);
    double sway = 0, behind = 0, most = -1.0;
    cell.widest = 0;
    for (int h = nh - 1; h >= 0; h--) {
      const double *a = &line[6 * h];
      double far = 0;
      for (int k = 0; k < np; k++) {
        const double r[3] = {pts[k][0] - a[0], pts[k][1] - a[1], pts[k][2] - a[2]};
        const double x[3] = {r[1] * a[5] - r[2] * a[4], r[2] * a[3] - r[0] * a[5], r[0] * a[4] - r[1] * a[3]};
        far = std::fmax(far, norm3(x));
      }
      const double arm = std::fmin(lever[h], far + behind), part = cell.w[h] * arm;
      sway += part;
      behind += cell.w[h] * lever[h];
      if (part > most) { most = part; cell.widest = h; }
    }
    cell.low = gap - sway;
    return gap > 0;  // (NaN: false)
  };
  int pair_evals = 0;
  return prune_bisect(nh, &pair_evals, budget, evals, kContactModelEvals, bound_cell) > 0;
}

// L: the layout the program is compiled from (the pairs stage 1b dropped are on no list and are not looked at again);
// tol, poison_slack, poison_rows: of the program's own filter bound; pair_budget: cell evaluations per pair.  Returns the
// cell evaluations spent.
int prune_contacts(const HostModel &m, const ModelLayout &L, double tol, double poison_slack, const std::vector<int> &poison_rows,
                   int pair_budget, GeomPairs *never) {
  never->clear();
  int evals = 0;
  const double need = kPruneSlack + 2.0 * tol + poison_slack;
  for (int k = 0; k < (int)L.mgeoms.size(); k++) {
    const int g = L.mgeoms[k];
    PruneChain c;
    if (!prune_chain(m, L, m.geom_bodyid[g], -1, &c)) continue;
    bool finite = true;
    for (int a = 0; a < 3; a++) finite = finite && std::isfinite(m.geom_size[3 * g + a]);
    if (!finite) continue;
    for (int sgeom : L.world_partners[k]) {
      if (std::find(poison_rows.begin(), poison_rows.end(), L.world_row[sgeom]) != poison_rows.end()) continue;
      PruneCore S;
      S.type = m.geom_type[sgeom];
      bool ok = true;
      for (int a = 0; a < 3; a++) {
        S.c[a] = L.st_gxpos[3 * sgeom + a];
        S.size[a] = m.geom_size[3 * sgeom + a];
        ok = ok && (S.type == GT_PLANE || std::isfinite(S.size[a]));
      }
      if (!ok) continue;
      for (int a = 0; a < 9; a++) S.R[a] = L.st_gxmat[9 * sgeom + a];
      PruneCore A;
      A.type = m.geom_type[g];
      A.size[0] = m.geom_size[3 * g];
      const double margin = std::fmax(m.geom_margin[g], m.geom_margin[sgeom]);
      if (contact_prove(m, c, g, S, A.radius() + S.radius() + margin, need, pair_budget, &evals))
        never->insert({std::min(g, sgeom), std::max(g, sgeom)});
    }
  }
  return std::min(evals, kContactModelEvals);
}

// ---- stage 2: ip / dp

// dp indices the float image treats specially (float_image)
struct BoundSites {
  std::vector<std::pair<size_t, int>> info_at;      // dp index -> int stored there (first 4 bytes)
  std::vector<size_t> sq_bound_at, plane_bound_at;  // cull bounds: squared distances, plane distances
};

// the world tables in front of dp: cull rows, four side by side per chunk (wc_at) with one spare chunk -- the
// kernels may prefetch ahead --, then the narrowphase rows
void emit_world_tables(const HostModel &m, const ModelLayout &L, std::vector<int> &ip, std::vector<double> &dp, BoundSites *sites) {
  const int nworld = L.nworld(), nwpad = (nworld + 3) / 4 * 4;
  ip[H_OFF_WCULL] = 0;
  ip[H_NWORLD] = nworld;
  ip[H_NWPAD] = nwpad;
  ip[H_OFF_WNARROW] = (nwpad + 4) * WC_LEN;
  dp.assign((size_t)ip[H_OFF_WNARROW] + (size_t)nworld * WN_LEN, 0.0);
  for (int w = 0; w < nworld; w++) {
    const int g = L.winfo[w] >> 8;
    const double *gmx = &L.st_gxmat[9 * g];
    double *rn = &dp[(size_t)ip[H_OFF_WNARROW] + (size_t)w * WN_LEN];
    for (int k = 0; k < 3; k++) {
      dp[wc_at(w, WC_POS + k)] = L.st_gxpos[3 * g + k];
      rn[WN_XAXIS + k] = gmx[3 * k + 0];
      rn[WN_YAXIS + k] = gmx[3 * k + 1];
      rn[WN_ZAXIS + k] = gmx[3 * k + 2];
      rn[WN_SIZE + k] = m.geom_size[3 * g + k];
    }
    const int32_t info[2] = {L.winfo[w], 0};
    memcpy(&dp[wc_at(w, WC_INFO)], info, sizeof(double));
    sites->info_at.push_back({(size_t)wc_at(w, WC_INFO), L.winfo[w]});
  }
}

// one moving geom (stage gk): its record, the cull rows of its static partners, the slot rows of its stored ones
void emit_geom(const HostModel &m, const ModelLayout &L, int gk, std::vector<int> &ip, std::vector<double> &dp, BoundSites *sites) {
  const int g = L.mgeoms[gk], nwpad = ip[H_NWPAD];
  const double *gp = &m.geom_pos[3 * g], *gq = &m.geom_quat[4 * g];
  int flags = 0;
  if (gp[0] == 0 && gp[1] == 0 && gp[2] == 0) flags |= GF_SAMEPOS;
  if (gq[0] == 1 && gq[1] == 0 && gq[2] == 0 && gq[3] == 0) flags |= GF_SAMEROT;
  unsigned long long wmask = 0, pmask = 0;
  for (int sgeom : L.world_partners[gk])
    (m.geom_type[sgeom] == GT_PLANE ? pmask : wmask) |= 1ull << L.world_row[sgeom];
  unsigned smask = 0;
  for (int k2 : L.stored_partners[gk]) smask |= 1u << (L.slot_of[k2] & 63);
  const int rec[G_SIZE] = {m.geom_type[g], flags, (int)dp.size(), L.slot_of[gk], g, (int)smask,
                           (int)(uint32_t)(wmask & 0xffffffffull), (int)(uint32_t)(wmask >> 32),
                           (int)(uint32_t)(pmask & 0xffffffffull), (int)(uint32_t)(pmask >> 32)};
  ip.insert(ip.end(), rec, rec + G_SIZE);
  const size_t swords_at = ip.size();
  ip.insert(ip.end(), MAX_SLOTS, 0);
  for (int k3 = 0; k3 < 3; k3++) dp.push_back(gp[k3]);
  for (int k4 = 0; k4 < 4; k4++) dp.push_back(gq[k4]);
  for (int k3 = 0; k3 < 3; k3++) dp.push_back(m.geom_size[3 * g + k3]);
  dp.push_back((double)g);  // GD_GEOMID
  dp.push_back(0.0);
  const double inf = std::numeric_limits<double>::infinity();
  // [nwpad] bounds, [nwpad] margins.  Rows that are no partner of this geom: -inf, so the queued culls need no enable mask
  const size_t wb = dp.size(), wm = wb + nwpad;
  dp.insert(dp.end(), nwpad, -inf);
  dp.insert(dp.end(), nwpad, 0.0);
  for (int sgeom : L.world_partners[gk]) {
    const bool plane = m.geom_type[sgeom] == GT_PLANE;
    const int w = L.world_row[sgeom];
    const PairBound pb = pair_bound(m, std::min(g, sgeom), std::max(g, sgeom), plane ? sgeom : -1);
    dp[wb + w] = pb.bound;
    dp[wm + w] = pb.margin;
    (plane ? sites->plane_bound_at : sites->sq_bound_at).push_back(wb + w);
  }
  // per register slot: bound, margin, the occupant's size[3] and geom id (GS_GEOMID)
  const size_t sb = dp.size(), sm = sb + MAX_SLOTS, ss = sm + MAX_SLOTS, sg = ss + 3 * MAX_SLOTS;
  dp.insert(dp.end(), MAX_SLOTS, inf);
  dp.insert(dp.end(), 4 * MAX_SLOTS, 0.0);
  dp.insert(dp.end(), MAX_SLOTS, -1.0);
  for (int k2 : L.stored_partners[gk]) {
    const int h = L.mgeoms[k2];
    const int s1 = L.slot_of[k2] & 63, s2 = (L.slot_of[k2] >> 6) & 63;
    const int g1 = std::min(g, h), g2 = std::max(g, h);
    const int first = (m.geom_type[g1] > m.geom_type[g2]) ? g2 : g1;
    ip[swords_at + s1] = s2 | (m.geom_type[h] << 12) | (first == h ? P_FIRST : 0);
    const PairBound pb = pair_bound(m, g1, g2, -1);  // (a moving geom is no plane: layout_moving)
    dp[sb + s1] = pb.bound;
    dp[sm + s1] = pb.margin;
    sites->sq_bound_at.push_back(sb + s1);
    for (int k3 = 0; k3 < 3; k3++) dp[ss + 3 * s1 + k3] = m.geom_size[3 * h + k3];
    dp[sg + s1] = (double)h;
  }
}

void emit_program(const HostModel &m, const ModelLayout &L, const std::vector<int> &qidx, const std::vector<double> &qbase,
                  std::vector<int> &ip, std::vector<double> &dp, BoundSites *sites) {
  const int nplan = (int)qidx.size(), nm = (int)L.mgeoms.size();
  ip.assign(H_SIZE, 0);
  ip[H_NPLAN] = nplan;
  ip[H_NSAVE] = L.nsave;
  ip[H_NSLOTS] = L.nslots;
  ip[H_NBODYOPS] = (int)L.order.size();
  emit_world_tables(m, L, ip, dp, sites);

  // column permutation: ascending qpos address (the order np.linalg.norm sums the full vector)
  ip[H_OFF_PERM] = (int)ip.size();
  {
    std::vector<int> perm(nplan);
    for (int c = 0; c < nplan; c++) perm[c] = c;
    std::sort(perm.begin(), perm.end(), [&](int a, int b) { return qidx[a] < qidx[b]; });
    for (int c : perm) ip.push_back(c);
  }

  ip[H_OFF_BODYOPS] = (int)ip.size();
  int gk = 0;  // index into mgeoms
  for (size_t k = 0; k < L.order.size(); k++) {
    const int b = L.order[k], p = m.body_parentid[b];
    const size_t base = ip.size();
    ip.resize(base + B_SIZE);
    ip[base + B_PARENT] = L.parent_src[k];
    ip[base + B_DOFF] = (int)dp.size();
    ip[base + B_BODYID] = b;
    ip[base + B_NJNT] = m.body_jntnum[b];
    ip[base + B_SAVE] = L.save_slot[b];
    for (int k3 = 0; k3 < 3; k3++) dp.push_back(m.body_pos[3 * b + k3]);
    for (int k4 = 0; k4 < 4; k4++) dp.push_back(m.body_quat[4 * b + k4]);
    if (L.parent_src[k] == PARENT_STATIC) {
      for (int k3 = 0; k3 < 3; k3++) dp.push_back(L.st_xpos[3 * p + k3]);
      for (int k4 = 0; k4 < 4; k4++) dp.push_back(L.st_xquat[4 * p + k4]);
      for (int k9 = 0; k9 < 9; k9++) dp.push_back(L.st_xmat[9 * p + k9]);
    }
    for (int j = 0; j < m.body_jntnum[b]; j++) {
      const int jid = m.body_jntadr[b] + j;
      const int qadr = m.jnt_qposadr[jid];
      const double *jp = &m.jnt_pos[3 * jid];
      ip.push_back(m.jnt_type[jid]);
      ip.push_back(L.col_of[qadr]);
      ip.push_back((jp[0] != 0 || jp[1] != 0 || jp[2] != 0) ? JF_POS_NONZERO : 0);
      ip.push_back((int)dp.size());
      for (int k3 = 0; k3 < 3; k3++) dp.push_back(m.jnt_axis[3 * jid + k3]);
      for (int k3 = 0; k3 < 3; k3++) dp.push_back(jp[k3]);
      dp.push_back(m.qpos0[qadr]);
      dp.push_back(qbase[qadr]);
    }
    int ngeom_here = 0;
    for (; gk < nm && m.geom_bodyid[L.mgeoms[gk]] == b; gk++, ngeom_here++) emit_geom(m, L, gk, ip, dp, sites);
    ip[base + B_NGEOM] = ngeom_here;
  }

  // the kernels prefetch one entry past the one they test: keep that read inside the tables
  ip.insert(ip.end(), 32, 0);
  dp.insert(dp.end(), 24, 0.0);
}

// ---- stage 3: binary32 error bound of the filter.  eps = 2^-24.  For every
// moving body b, by induction along the chain (every operation of run_config_queued counted with
// its worst-case rounding; fused multiply-adds only lower these):
//   rot(b) <= rot(parent) + (20 + 42 * hinges(b)) eps          orientation error, radians
//   pos(b) <= posA(b) + posB(b) * C                            position error, metres, where C
//             bounds every moving coordinate magnitude (enforced per lane: FC_MAXCOORD), and
//   posA(b) = posA(parent) + L_b (rot(parent) + 8 eps) + 3 eps L_b + sum_hinges 2 |jnt_pos| (rot(b) + 8 eps)
//   posB(b) = posB(parent) + sqrt(3) eps (1 + slides(b) + 2 offcentre_hinges(b))
// A geom adds |lpos| (rot + 8 eps) + extent (rot + 24 eps) + 2 eps |size| and sqrt(3) eps C; a static
// geom is off by the rounding of its constants; evaluating a narrowphase formula on binary32
// poses adds 16 eps (pair scale) + 4 eps C.  Signed distances are 1-Lipschitz in every point of
// either geom, so |distance32 - distance64| <= E = A + B C over all enabled pairs.
// Reads the tolerance asked for (and whether the caller or the default asked); appends the filter's constants to dp
// (ip[H_OFF_FCONST]).
FilterBound filter_error_bound(const HostModel &m, const ModelLayout &L, float tol_req, bool tol_user, std::vector<int> &ip,
                               std::vector<double> &dp) {
  FilterBound fb;
  const int nb = m.nbody, ng = m.ngeom, nm = (int)L.mgeoms.size();
  const double eps = std::ldexp(1.0, -24);
  const double r3 = std::sqrt(3.0);
  std::vector<double> rot(nb, 0.0), posA(nb, 0.0), posB(nb, 0.0);
  for (int b = 0; b < nb; b++)
    if (L.body_static[b]) { rot[b] = 2 * eps; posA[b] = r3 * eps * norm3(&L.st_xpos[3 * b]); }
  for (int b : L.order) {
    const int p = m.body_parentid[b];
    int hinges = 0, slides = 0, off = 0;
    double jp = 0;
    for (int j = 0; j < m.body_jntnum[b]; j++) {
      const int jid = m.body_jntadr[b] + j;
      if (m.jnt_type[jid] == JT_HINGE) {
        hinges++;
        const double l = norm3(&m.jnt_pos[3 * jid]);
        if (l > 0) { off++; jp += l; }
      } else {
        slides++;
      }
    }
    const double Lb = norm3(&m.body_pos[3 * b]);
    rot[b] = rot[p] + (20.0 + 42.0 * hinges) * eps;
    posA[b] = posA[p] + Lb * (rot[p] + 8 * eps) + 3 * eps * Lb + 2 * jp * (rot[b] + 8 * eps);
    posB[b] = posB[p] + r3 * eps * (1 + slides + 2 * off);
  }
  auto extent = [&](int g) {  // farthest point of the geom from its frame origin along rotating directions
    const double *sz = &m.geom_size[3 * g];
    if (m.geom_type[g] == GT_CAPSULE) return sz[1];
    if (m.geom_type[g] == GT_BOX) return norm3(sz);
    return 0.0;
  };
  std::vector<double> gA(ng, 0.0), gB(ng, 0.0);
  std::vector<char> poisoned(ng, 0);
  const double tolh_req = 0.5 * tol_req;
  for (int g = 0; g < ng; g++) {
    const int b = m.geom_bodyid[g];
    const double lp = norm3(&m.geom_pos[3 * g]), sz = norm3(&m.geom_size[3 * g]);
    if (L.geom_static[g]) {
      gA[g] = r3 * eps * (norm3(&L.st_gxpos[3 * g]) + extent(g)) + 2 * eps * sz;
      // a static geom whose own constants do not fit binary32 within an eighth of the band: its
      // narrowphase rows are NaN in the float tables, so every pair that passes its (widened)
      // cull comes out undecided and is settled by the float64 pair kernel
      if (gA[g] > 0.25 * tolh_req) { poisoned[g] = 1; fb.npoisoned++; }
    } else {
      gA[g] = posA[b] + lp * (rot[b] + 8 * eps) + extent(g) * (rot[b] + 24 * eps) + 2 * eps * sz;
      gB[g] = posB[b] + r3 * eps;
    }
  }
  double A = 0, B = 0;
  for (int k = 0; k < nm; k++) {
    const int g = L.mgeoms[k];
    auto pair = [&](int h) {
      if (poisoned[h]) return;
      const double scale = m.geom_rbound[g] + m.geom_rbound[h] + std::fmax(m.geom_margin[g], m.geom_margin[h]) +
                           (m.geom_type[h] == GT_PLANE ? norm3(&L.st_gxpos[3 * h]) : 0.0);
      A = std::fmax(A, gA[g] + gA[h] + 16 * eps * scale);
      B = std::fmax(B, gB[g] + gB[h] + 4 * eps);
    };
    for (int sgeom : L.world_partners[k]) pair(sgeom);
    for (int k2 : L.stored_partners[k]) pair(L.mgeoms[k2]);
  }
  fb.ferr_a = A;
  fb.ferr_b = B;
  // half the band is the error budget: E(C) = A + B C <= tol / 2.  A default tolerance grows with
  // the model's floor; one the caller asked for is kept, and if the floor does not fit under it
  // the filter steps aside for this model (exact path only).
  double tol = tol_req;
  fb.usable = true;
  if (A > 0.4 * tol) {
    if (tol_user) fb.usable = false;
    else tol = A / 0.4;
    if (!(tol < 1e-2)) fb.usable = false;  // a band of centimetres decides nothing useful
  }
  fb.tol = (float)tol;
  // (a candidate record of the filter's queues carries its geom's table offset in 16 bits -- the other half of the word
  //  is the candidate's certificate margin, mjpl_device.h: queue_drain --: a table of 64 K entries or more, far beyond
  //  any model the slot file holds, takes the exact path)
  if (dp.size() + 64 >= 65536) fb.usable = false;
  double maxc = (B > 0) ? (0.5 * tol - A) / B : 1e6;
  maxc = std::fmin(std::fmax(maxc, 0.0), 1e6);
  fb.fmax_coord = fb.usable ? maxc : 0.0;
  ip[H_OFF_FCONST] = (int)dp.size();
  double fc[FC_SIZE] = {0};
  fc[FC_MAXCOORD] = fb.fmax_coord;
  fc[FC_MAXANGLE] = kFilterMaxAngle;
  dp.insert(dp.end(), fc, fc + FC_SIZE);
  // NaN rows: written into the float image
  for (int g = 0; g < ng; g++)
    if (poisoned[g]) fb.poison_rows.push_back(L.world_row[g]);
  return fb;
}

// a poisoned static geom's own rounding may exceed the band: every cull bound of the float image is widened by that, too
double poison_widening(const std::vector<int> &ip, const std::vector<double> &dp, const FilterBound &fb) {
  double poison_slack = 0;
  for (int w : fb.poison_rows) {
    const double *wt = &dp[(size_t)ip[H_OFF_WCULL]];
    const double rc[3] = {wt[wc_at(w, 0)], wt[wc_at(w, 1)], wt[wc_at(w, 2)]};
    const double *rn = &dp[(size_t)ip[H_OFF_WNARROW] + (size_t)w * WN_LEN];
    const double mag = std::fabs(rc[0]) + std::fabs(rc[1]) + std::fabs(rc[2]) + std::fabs(rn[WN_SIZE]) +
                       std::fabs(rn[WN_SIZE + 1]) + std::fabs(rn[WN_SIZE + 2]);
    poison_slack = std::fmax(poison_slack, 4 * std::ldexp(1.0, -24) * mag);
  }
  return poison_slack;
}

// ---- stage 4: the filter's float32 image: same offsets; cull bounds widened by the tolerance so that
// a pair culled in float32 is certainly culled (or contact-free) in float64
void float_image(const std::vector<int> &ip, const std::vector<double> &dp, const BoundSites &sites, const FilterBound &fb,
                 std::vector<float> &fp) {
  fp.resize(dp.size());
  for (size_t k = 0; k < dp.size(); k++) fp[k] = (float)dp[k];
  const double tol = fb.tol, poison_slack = poison_widening(ip, dp, fb);
  for (size_t k : sites.sq_bound_at)
    if (std::isfinite(dp[k])) {
      const double r = std::sqrt(dp[k]) + tol + poison_slack;
      fp[k] = (float)(r * r * (1.0 + 1e-6));
    }
  for (size_t k : sites.plane_bound_at)
    if (std::isfinite(dp[k])) fp[k] = (float)(dp[k] + tol + poison_slack + 1e-6 * std::fabs(dp[k]));
  for (auto &kv : sites.info_at) memcpy(&fp[kv.first], &kv.second, sizeof(float));
  // the whole narrowphase row (axes and sizes; the position belongs to the cull table): every
  // routine then computes NaN and classifies the pair as undecided
  for (int w : fb.poison_rows)
    for (int k = 0; k < WN_LEN; k++) fp[(size_t)ip[H_OFF_WNARROW] + (size_t)w * WN_LEN + k] = std::numeric_limits<float>::quiet_NaN();
}

// ---- stage 5: identity of the compiled program: what a per-model specialised library is keyed by
uint64_t hash_program(const ModelLayout &L, const std::vector<int> &ip, const std::vector<float> &fp, const std::vector<double> &dp,
                      const GeomPairs &never_touch) {
  Fnv1a f;
  f.mix(ip.data(), ip.size() * sizeof(int));
  f.mix(fp.data(), fp.size() * sizeof(float));
  // the float64 table as well: the generated exact pair re-check (ExactSpec::fk_pair) carries ITS values
  // as literals, and two programs may share a binary32 image while their float64 constants differ
  f.mix(dp.data(), dp.size() * sizeof(double));
  const int shape[4] = {L.maxs, L.wbox ? 1 : 0, L.mbox ? 1 : 0, MJPL_SPEC_ABI};
  f.mix(shape, sizeof(shape));
  f.mix_stamp();
  // the pairs a per-program library leaves out of its generated check (stage 1c), only when there are any: a model where
  // nothing is proved keeps the hash it had without the stage
  if (!never_touch.empty()) {
    f.mixi(-3);
    for (const auto &gp : never_touch) { f.mixi(gp.first); f.mixi(gp.second); }
  }
  return f.h;
}

// ---- stage 6: identity of the ROBOT alone, and the cull table a scene-generic library reads.
// Everything the generated code of such a library carries as literals goes into the robot hash: the moving
// bodies with their constants, joints (planning column or constant), geoms, register slots and self
// pairs with their bounds, tolerance, kernel shape.  Nothing of the static geoms: those reach the code
// through the scene table (scene_table).
uint64_t hash_robot(const HostModel &m, const ModelLayout &L, const std::vector<double> &qbase, int nplan, float tol) {
  const int nm = (int)L.mgeoms.size();
  Fnv1a f;
  f.mixi(nplan); f.mixi(L.maxs); f.mixi(L.nslots); f.mixi(L.nsave); f.mixi(MJPL_SPEC_ABI); f.mixi(kSceneRows);
  f.mix_stamp();
  f.mix(&tol, sizeof(tol));
  int gk = 0;
  for (size_t k = 0; k < L.order.size(); k++) {
    const int b = L.order[k], p = m.body_parentid[b];
    f.mixi(L.parent_src[k]);
    f.mixd(&m.body_pos[3 * b], 3); f.mixd(&m.body_quat[4 * b], 4);
    if (L.parent_src[k] == PARENT_STATIC) { f.mixd(&L.st_xpos[3 * p], 3); f.mixd(&L.st_xquat[4 * p], 4); f.mixd(&L.st_xmat[9 * p], 9); }
    f.mixi(m.body_jntnum[b]); f.mixi(L.save_slot[b]);
    for (int j = 0; j < m.body_jntnum[b]; j++) {
      const int jid = m.body_jntadr[b] + j, qadr = m.jnt_qposadr[jid];
      f.mixi(m.jnt_type[jid]); f.mixi(L.col_of[qadr]);
      f.mixd(&m.jnt_axis[3 * jid], 3); f.mixd(&m.jnt_pos[3 * jid], 3); f.mixd(&m.qpos0[qadr], 1);
      const double qc = L.col_of[qadr] < 0 ? qbase[qadr] : 0.0;
      f.mixd(&qc, 1);
    }
    for (; gk < nm && m.geom_bodyid[L.mgeoms[gk]] == b; gk++) {
      const int g = L.mgeoms[gk];
      f.mixi(m.geom_type[g]); f.mixi(L.slot_of[gk]);
      f.mixd(&m.geom_pos[3 * g], 3); f.mixd(&m.geom_quat[4 * g], 4); f.mixd(&m.geom_size[3 * g], 3);
      f.mixd(&m.geom_rbound[g], 1); f.mixd(&m.geom_margin[g], 1);
      for (int k2 : L.stored_partners[gk]) { f.mixi(k2); f.mixi(L.slot_of[k2]); }
      f.mixi(-1);
    }
    f.mixi(-2);
  }
  return f.h;
}

// does the program satisfy what a scene-generic library assumes?  `queued`: the queued filter kernels serve it
// (a robot with moving boxes, or 17 .. 24 stored geoms: the 24-slot queued build has generated code, too)
bool scene_generic_ok(const ModelLayout &L, const FilterBound &fb, bool queued) {
  const int nm = (int)L.mgeoms.size(), nplanes = L.nplanes;
  bool ok = queued && fb.usable && nplanes <= kScenePlaneRows && L.nworld() - nplanes <= kSceneRows - kScenePlaneRows &&
            nm <= kSceneMaxStages && nm > 0;
  for (int k = 1; k < nm && ok; k++) ok = L.mgeoms[k] == L.mgeoms[0] + k;  // (the pair re-check counts geoms from the first moving one)
  return ok;
}

// The scene table: a header, then for every moving geom kSceneRows cull rows [a0 a1 a2 thr] followed by
// kSceneRows descriptor words: a plane partner (rows 0, 1) passes its cull when a . c <= thr (a =
// normal), any other (rows 2 ..) when |c|^2 + a . c <= thr (a = -2 X: the expanded form, threshold
// raised by the form's rounding bound for a centre within the geom's reach); the descriptor says what a
// candidate of that pair is queued as.  Rows that are no pair of the geom never pass (thr = -inf).
// `box_queue`: a moving box's candidates go to the box queue (mjpl_engine::filter_mbox).
void scene_table(const HostModel &m, const ModelLayout &L, const FilterBound &fb, const std::vector<int> &ip,
                 const std::vector<float> &fp, bool box_queue, std::vector<float> &scene) {
  const int nb = m.nbody, ng = m.ngeom, nworld = L.nworld(), nplanes = L.nplanes;
  scene.assign(scene_floats((int)L.mgeoms.size()), 0.0f);
  auto seti = [&](size_t at, int v) { memcpy(&scene[at], &v, sizeof(float)); };
  const double u24 = std::ldexp(1.0, -24);
  auto round_up = [](double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
    return f;
  };
  // how far from the origin a moving geom's centre can be while its lane is alive (specialise.py: the same)
  const double box_reach = std::sqrt(3.0) * (double)(float)fb.fmax_coord;
  std::vector<double> breach(nb, 0.0);
  for (int b : L.order) {
    const int p = m.body_parentid[b];
    double r = (L.body_static[p] ? norm3(&L.st_xpos[3 * p]) : breach[p]) + norm3(&m.body_pos[3 * b]);
    for (int j = 0; j < m.body_jntnum[b]; j++) {
      const int jid = m.body_jntadr[b] + j;
      if (m.jnt_type[jid] == JT_SLIDE) r = std::numeric_limits<double>::infinity();
      else r += 2.0 * norm3(&m.jnt_pos[3 * jid]);
    }
    breach[b] = std::fmin(r, box_reach);
  }
  // [0] planes (0 .. 2: the last rows), [1] first pair of rows in use, [2] nwpad, [3] offset of the narrowphase table
  // The rows of a geom are filled from the END: the planes last, the bounded geoms below them; the code is one
  // straight line over all kSceneRows rows, entered at the first pair of rows that holds anything ([1]).
  const int nbounded = nworld - nplanes;
  const int first_row = std::min(kSceneRows - 2, (kSceneRows - nplanes - nbounded) & ~1);
  seti(0, nplanes); seti(1, first_row);
  seti(2, ip[H_NWPAD]); seti(3, ip[H_OFF_WNARROW]);
  scene[4] = (float)fb.fmax_coord;
  scene[5] = kFilterMaxAngle;
  int gk = 0, pc = ip[H_OFF_BODYOPS];
  for (size_t k = 0; k < L.order.size(); k++) {
    const int b = L.order[k];
    const int njnt = ip[pc + B_NJNT], ngeom_here = ip[pc + B_NGEOM];
    pc += B_SIZE + njnt * J_SIZE;
    for (int gi = 0; gi < ngeom_here; gi++, gk++) {
      const int g = L.mgeoms[gk], gtype = m.geom_type[g], gdoff = ip[pc + G_DOFF];
      pc += G_SIZE + MAX_SLOTS;
      seti(8 + gk, gdoff);
      const double reach = breach[b] + norm3(&m.geom_pos[3 * g]);
      std::set<int> partners(L.world_partners[gk].begin(), L.world_partners[gk].end());
      float *rows = &scene[(size_t)kSceneHeader + (size_t)gk * kSceneStageFloats];
      float *descs = rows + (size_t)kSceneRows * 4;
      for (int r0 = 0; r0 < kSceneRows; r0++) rows[(size_t)r0 * 4 + 3] = -std::numeric_limits<float>::infinity();
      for (int pass = 0; pass < 2; pass++) {  // the planes in the last rows, the others below them
        int r = pass == 0 ? kSceneRows - nplanes : kSceneRows - nplanes - nbounded;
        for (int sgeom = 0; sgeom < ng; sgeom++) {
          if (!L.geom_static[sgeom] || L.world_row[sgeom] < 0) continue;
          const int w = L.world_row[sgeom], ptype = L.winfo[w] & 255;
          if ((ptype == GT_PLANE) != (pass == 0)) continue;
          float *row = rows + (size_t)r * 4;
          float *dword = descs + r;
          r++;
          if (!partners.count(sgeom)) continue;  // (not a pair of this geom: a row that never passes)
          const double X[3] = {(double)fp[wc_at(w, 0)], (double)fp[wc_at(w, 1)], (double)fp[wc_at(w, 2)]};
          const double bound = (double)fp[(size_t)gdoff + GD_WBOUND + w];
          int desc;
          if (ptype == GT_PLANE) {
            const float *rw = &fp[(size_t)ip[H_OFF_WNARROW] + (size_t)w * WN_LEN];
            const double n[3] = {(double)rw[WN_ZAXIS], (double)rw[WN_ZAXIS + 1], (double)rw[WN_ZAXIS + 2]};
            const double off = n[0] * X[0] + n[1] * X[1] + n[2] * X[2];
            for (int c = 0; c < 3; c++) row[c] = (float)n[c];
            // three fused multiply-adds on a centre within `reach`: each rounds by at most u (reach + |n . p0| + |bound|)
            row[3] = std::isfinite(reach) ? round_up(bound + off + 4.0 * u24 * (1.01 * reach + std::fabs(off) + std::fabs(bound)))
                                          : std::numeric_limits<float>::infinity();
            // (bit 15: the candidate goes to the box queue -- a static box, or ANY partner of a moving box, whose
            //  records carry whole frames)
            desc = EK_PLANE | (w << 2) | (GT_PLANE << 10) | (1 << 14) | ((gtype == GT_BOX && box_queue ? 1 : 0) << 15);
          } else {
            const double nx = std::sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
            for (int c = 0; c < 3; c++) row[c] = (float)(-2.0 * X[c]);
            // (the allowance of specialise.py: expanded_threshold)
            const double allow = 8.0 * u24 * (1.01 * reach + nx) * (1.01 * reach + nx);
            row[3] = std::isfinite(reach) ? round_up(bound - (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) + allow)
                                          : std::numeric_limits<float>::infinity();
            if (!std::isfinite(bound)) row[3] = (float)bound;
            const int pgid = L.winfo[w] >> 8;
            const int pfirst = (ptype < gtype || (ptype == gtype && pgid < g)) ? 1 : 0;
            desc = EK_STATIC | (w << 2) | (ptype << 10) | (pfirst << 14) |
                   (((ptype == GT_BOX || (gtype == GT_BOX && box_queue)) ? 1 : 0) << 15);
          }
          memcpy(dword, &desc, sizeof(float));
        }
      }
    }
  }
}

// Stage 1b's driver: e->pruned from the program with every enabled pair.  That program is compiled as far as its error
// bound, because the proof's margin covers the band IT would run with -- the reduced program's band is no wider (the
// floor of filter_error_bound is a maximum over the pairs left).  Nothing the result depends on changes with the
// planning selection, so it is kept until the switch or the tolerance asked for changes.
int find_pruned_pairs(mjpl_engine *e) {
  if (!e->prune_pairs) {
    e->pruned.clear();
    e->pruned_valid = false;
    return MJPL_OK;
  }
  if (e->pruned_valid && e->pruned_level == e->prune_pairs && e->pruned_tol_req == e->filter_tol_req &&
      e->pruned_tol_user == e->filter_tol_user)
    return MJPL_OK;
  ModelLayout full;
  MJPL_TRY(layout_model(e->m, e->allowed, GeomPairs(), e->qidx, &full));
  std::vector<int> ip;
  std::vector<double> dp;
  BoundSites sites;
  emit_program(e->m, full, e->qidx, e->qbase, ip, dp, &sites);
  const FilterBound fb = filter_error_bound(e->m, full, e->filter_tol_req, e->filter_tol_user, ip, dp);
  // (a filter that steps aside for the full program may serve the reduced one: then with the band asked for, or a default
  //  one below the centimetre filter_error_bound gives up at)
  const double tol = fb.usable ? fb.tol : (e->filter_tol_user ? e->filter_tol_req : 1e-2);
  e->prune_evals = prune_pairs(e->m, full, tol, poison_widening(ip, dp, fb), e->prune_pairs >= 2, &e->pruned);
  e->pruned_valid = true;
  e->pruned_level = e->prune_pairs;
  e->pruned_tol_req = e->filter_tol_req;
  e->pruned_tol_user = e->filter_tol_user;
  return MJPL_OK;
}

// Stage 1c's driver: e->never_touch from the layout the program is compiled from and its own filter bound (a model the
// filter does not serve runs no generated check: nothing to leave out).  Like stage 1b's decisions the set does not change
// with the planning selection: kept until the switches, the dropped pairs or the band change.
void find_never_touch(mjpl_engine *e) {
  if (!e->prune_contacts || !e->fb.usable) {
    e->never_touch.clear();
    e->never_valid = false;
    return;
  }
  const double poison_slack = poison_widening(e->ip, e->dp, e->fb);
  if (e->never_valid && e->never_level == e->prune_contacts && e->never_from == e->pruned && e->never_tol == (double)e->fb.tol &&
      e->never_poison_slack == poison_slack && e->never_poison_rows == e->fb.poison_rows)
    return;
  const int budget = e->prune_contacts >= 2 ? e->prune_contacts : kContactPairEvals;
  e->prune_contact_evals = prune_contacts(e->m, e->lay, (double)e->fb.tol, poison_slack, e->fb.poison_rows, budget, &e->never_touch);
  e->never_valid = true;
  e->never_level = e->prune_contacts;
  e->never_from = e->pruned;
  e->never_tol = (double)e->fb.tol;
  e->never_poison_slack = poison_slack;
  e->never_poison_rows = e->fb.poison_rows;
}

// Stages 1 to 6: the engine's host tables, bound and hashes from its model, allowed pairs, planning selection and
// tolerance.  No HIP call, no device: mjpl_program_dump ends here; e->scene is non-empty exactly when the program
// satisfies what a scene-generic library assumes.
int compile_host(mjpl_engine *e) {
  const HostModel &m = e->m;
  MJPL_TRY(find_pruned_pairs(e));
  MJPL_TRY(layout_model(m, e->allowed, e->pruned, e->qidx, &e->lay));
  BoundSites sites;
  emit_program(m, e->lay, e->qidx, e->qbase, e->ip, e->dp, &sites);
  e->fb = filter_error_bound(m, e->lay, e->filter_tol_req, e->filter_tol_user, e->ip, e->dp);
  float_image(e->ip, e->dp, sites, e->fb, e->fp);
  find_never_touch(e);
  e->program_hash = hash_program(e->lay, e->ip, e->fp, e->dp, e->never_touch);
  e->robot_hash = hash_robot(m, e->lay, e->qbase, (int)e->qidx.size(), e->fb.tol);
  e->scene.clear();
  if (scene_generic_ok(e->lay, e->fb, !e->immediate()))
    scene_table(m, e->lay, e->fb, e->ip, e->fp, e->filter_mbox(), e->scene);
  return MJPL_OK;
}

// ---- the host halves of the create-time tables

// The candidate pairs of mj_collision (pair_candidate), allowed body pairs INCLUDED: the rows the caller sees
// (e->ct_*: smaller geom type first) and the kernel's records (mjpl_contacts.h: CI_* / CD_*).  A record restates
// what run_config tests for the pair: cur = the moving geom it places later, its partner, pfirst, margin and cull
// bound.  Depends on the model only (of the layout it reads geom_static, stage_of and world_row, which no planning
// selection changes): called once, at mjpl_create.
void build_contact_table(mjpl_engine *e, std::vector<int> &ip, std::vector<double> &dp) {
  const HostModel &m = e->m;
  const ModelLayout &L = e->lay;
  const int ng = m.ngeom;
  constexpr int kGeomHfield = 1;
  e->ct_g1.clear(); e->ct_g2.clear(); e->ct_allowed.clear();
  e->ct_unsupported = -1;
  for (int g1 = 0; g1 < ng; g1++)
    for (int g2 = g1 + 1; g2 < ng; g2++) {
      if (!pair_candidate(m, g1, g2)) continue;
      const int t1 = m.geom_type[g1], t2 = m.geom_type[g2];
      // (plane-hfield has no collision function either; the compiler refuses a height field unless the pair is allowed)
      if (std::min(t1, t2) == GT_PLANE && std::max(t1, t2) == kGeomHfield) continue;
      const int p = (int)e->ct_g1.size();
      e->ct_g1.push_back(t1 > t2 ? g2 : g1);
      e->ct_g2.push_back(t1 > t2 ? g1 : g2);
      e->ct_allowed.push_back(pair_allowed(m, e->allowed, g1, g2) ? 1 : 0);
      // (one geom is moving: both static means both welded to the world, filtered above)
      const bool s1 = L.geom_static[g1], s2 = L.geom_static[g2];
      int cur, par;
      if (s1 || s2) { cur = s1 ? g2 : g1; par = s1 ? g1 : g2; }
      else { cur = L.stage_of[g1] > L.stage_of[g2] ? g1 : g2; par = cur == g1 ? g2 : g1; }
      const int tcur = m.geom_type[cur], tpar = m.geom_type[par];
      if (e->ct_unsupported < 0 && (!type_supported(tcur) || !type_supported(tpar) || tcur == GT_PLANE)) e->ct_unsupported = p;
      const bool pstatic = L.geom_static[par] != 0;
      const bool pfirst = (tpar < tcur) || (tpar == tcur && par < cur);
      int rec[CI_LEN] = {0};
      rec[CI_CUR] = cur;
      rec[CI_PAR] = pstatic ? L.world_row[par] : par;
      rec[CI_TCUR] = tcur;
      rec[CI_TPAR] = tpar;
      rec[CI_FLAGS] = (pfirst ? CF_PFIRST : 0) | (pstatic ? CF_STATIC : 0);
      rec[CI_PARID] = par;
      ip.insert(ip.end(), rec, rec + CI_LEN);
      const PairBound pb = pair_bound(m, g1, g2, tpar == GT_PLANE ? par : -1);
      double d[CD_LEN] = {0};
      d[CD_MARGIN] = pb.margin;
      d[CD_BOUND] = pb.bound;
      for (int k = 0; k < 3; k++) {
        d[CD_SCUR + k] = m.geom_size[3 * cur + k];
        d[CD_SPAR + k] = m.geom_size[3 * par + k];
      }
      dp.insert(dp.end(), d, d + CD_LEN);
    }
}

// The distance table beside the candidate table (mjpl_distance.h: DT_*): rb1 + rb2 and the allowed flag per
// pair.  Depends on the model only: called once, at mjpl_create.
std::vector<double> build_distance_table(const mjpl_engine *e) {
  const int P = (int)e->ct_g1.size();
  std::vector<double> dt((size_t)P * DT_LEN);
  for (int p = 0; p < P; p++) {
    const int g1 = e->ct_g1[p], g2 = e->ct_g2[p];
    // (a plane partner's bound is the half-space itself: only the other geom's radius counts)
    const double rb1 = e->m.geom_type[g1] == GT_PLANE ? 0.0 : e->m.geom_rbound[g1];
    const double rb2 = e->m.geom_type[g2] == GT_PLANE ? 0.0 : e->m.geom_rbound[g2];
    dt[(size_t)p * DT_LEN + DT_RBSUM] = rb1 + rb2;
    dt[(size_t)p * DT_LEN + DT_ALLOWED] = e->ct_allowed[p] ? 1.0 : 0.0;
  }
  return dt;
}

// DFS entry / exit times of the body tree (children in id order): body a is b or above it iff
// tin[a] <= tin[b] < tout[a]
void body_dfs_times(const HostModel &m, std::vector<int> &tin, std::vector<int> &tout) {
  const int nb = m.nbody;
  std::vector<std::vector<int>> kids(nb);
  for (int b = 1; b < nb; b++) kids[m.body_parentid[b]].push_back(b);
  tin.assign(nb, 0);
  tout.assign(nb, 0);
  std::vector<int> stack = {0};
  std::vector<size_t> next(nb, 0);
  int clock = 0;
  tin[0] = clock++;
  while (!stack.empty()) {
    const int b = stack.back();
    if (next[b] < kids[b].size()) {
      const int k = kids[b][next[b]++];
      tin[k] = clock++;
      stack.push_back(k);
    } else {
      tout[b] = clock;
      stack.pop_back();
    }
  }
}

// The tables of k_distance<DM_GRAD> (mjpl_distance_grad.h): per planning column its joint's body, model joint id,
// the number of later joints on that body and the body's subtree as DFS times; per model joint its type, axis,
// position and where its dq comes from (as the FK program computes it); per geom the DFS entry time of its body.
// Depends on the model and the planning selection: made at mjpl_create and by mjpl_set_planning.
int build_grad_table(const mjpl_engine *e, std::vector<double> &t) {
  const HostModel &m = e->m;
  const std::vector<int> &col_of = e->lay.col_of;
  const int nplan = (int)e->qidx.size(), nj = m.njnt, ng = m.ngeom, nb = m.nbody;
  std::vector<int> tin, tout;
  body_dfs_times(m, tin, tout);
  std::vector<int> jnt_body(nj, 0);
  for (int b = 0; b < nb; b++)
    for (int j = 0; j < m.body_jntnum[b]; j++) jnt_body[m.body_jntadr[b] + j] = b;
  t.assign((size_t)nplan * GC_LEN + (size_t)nj * JR_LEN + ng, 0.0);
  double *gc = t.data(), *jr = gc + (size_t)nplan * GC_LEN, *gt = jr + (size_t)nj * JR_LEN;
  for (int j = 0; j < nj; j++) {
    const int qadr = m.jnt_qposadr[j];
    double *r = jr + (size_t)j * JR_LEN;
    r[JR_TYPE] = m.jnt_type[j];
    for (int k = 0; k < 3; k++) {
      r[JR_AXIS + k] = m.jnt_axis[3 * j + k];
      r[JR_POS + k] = m.jnt_pos[3 * j + k];
    }
    r[JR_COL] = col_of[qadr];
    r[JR_Q0] = col_of[qadr] >= 0 ? m.qpos0[qadr] : e->qbase[qadr] - m.qpos0[qadr];  // (the FK's qv - jd[6])
  }
  for (int c = 0; c < nplan; c++) {
    int j = -1;
    for (int k = 0; k < nj; k++)
      if (m.jnt_qposadr[k] == e->qidx[c]) j = k;
    if (j < 0) return fail(MJPL_E_JOINT, "planning column %d names qpos %d, which no joint owns", c, e->qidx[c]);
    const int b = jnt_body[j];
    double *r = gc + (size_t)c * GC_LEN;
    r[GC_BODY] = b;
    r[GC_JNT] = j;
    r[GC_NLATER] = m.body_jntadr[b] + m.body_jntnum[b] - 1 - j;
    r[GC_TIN] = tin[b];
    r[GC_TOUT] = tout[b];
  }
  for (int g = 0; g < ng; g++) gt[g] = tin[m.geom_bodyid[g]];
  return MJPL_OK;
}

// The pair lever table of k_distance<DM_SWEEP> (mjpl_distance.h): W[p][c] bounds how far one
// unit of planning column c can change the distance of candidate pair p.  rho_c(g), the lever of a planning hinge c
// for a geom g below it: the longest the chain can stretch from the hinge's anchor to the geom's centre -- body
// offsets, 2 |jnt_pos| per hinge passed, a slide held at its base as |qbase - q0|, a planning slide as
// max(|lo - q0|, |hi - q0|) (+inf without finite bounds), |geom_pos| -- plus geom_rbound[g]; a planning slide above g
// has lever 1.  W[p][c] is the lever for the one geom of the pair that c moves, 0 when it moves both or neither.
// lo, hi: bounds per planning column, either may be null (none).  Depends on the model, the planning selection and
// the bounds; not part of the hashed program.
std::vector<double> build_sweep_table(const mjpl_engine *e, const double *lo, const double *hi) {
  const HostModel &m = e->m;
  const std::vector<int> &col_of = e->lay.col_of;
  const int nplan = (int)e->qidx.size(), nb = m.nbody, P = (int)e->ct_g1.size();
  auto norm3 = [](const double *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
  // per body: the stretch from every planning hinge above it to the body's origin (-1: not above), and the planning
  // slides above it
  std::vector<double> reach((size_t)nb * nplan, -1.0);
  std::vector<char> slide((size_t)nb * nplan, 0);
  for (int b = 1; b < nb; b++) {
    double *r = &reach[(size_t)b * nplan];
    char *s = &slide[(size_t)b * nplan];
    const int parent = m.body_parentid[b];
    const double blen = norm3(&m.body_pos[3 * b]);
    for (int c = 0; c < nplan; c++) {
      r[c] = reach[(size_t)parent * nplan + c];
      s[c] = slide[(size_t)parent * nplan + c];
      if (r[c] >= 0) r[c] += blen;
    }
    for (int k = 0; k < m.body_jntnum[b]; k++) {
      const int j = m.body_jntadr[b] + k, qadr = m.jnt_qposadr[j], col = col_of[qadr];
      const double jp = norm3(&m.jnt_pos[3 * j]), q0 = m.qpos0[qadr];
      double add = 2.0 * jp;  // a hinge: the body's origin moves by at most twice its offset
      if (m.jnt_type[j] == JT_SLIDE && col < 0) add = std::fabs(e->qbase[qadr] - q0);  // held at its base
      if (m.jnt_type[j] == JT_SLIDE && col >= 0)  // planned: its travel inside the bounds
        add = std::max(std::fabs((lo ? lo[col] : -INFINITY) - q0), std::fabs((hi ? hi[col] : INFINITY) - q0));
      for (int c = 0; c < nplan; c++)
        if (r[c] >= 0) r[c] += add;
      if (col >= 0) {
        if (m.jnt_type[j] == JT_SLIDE) s[col] = 1;
        else r[col] = jp;
      }
    }
  }
  // rho_c(g), 0 when c is not above g
  auto lever = [&](int g, int c) {
    const int b = m.geom_bodyid[g];
    if (slide[(size_t)b * nplan + c]) return 1.0;
    const double r = reach[(size_t)b * nplan + c];
    return r < 0 ? 0.0 : r + norm3(&m.geom_pos[3 * g]) + m.geom_rbound[g];
  };
  std::vector<int> tin, tout, col_body(nplan, 0);
  body_dfs_times(m, tin, tout);
  for (int b = 0; b < nb; b++)
    for (int k = 0; k < m.body_jntnum[b]; k++) {
      const int col = col_of[m.jnt_qposadr[m.body_jntadr[b] + k]];
      if (col >= 0) col_body[col] = b;
    }
  auto above = [&](int c, int g) {
    const int a = col_body[c], b = m.geom_bodyid[g];
    return tin[a] <= tin[b] && tin[b] < tout[a];
  };
  std::vector<double> W((size_t)P * nplan, 0.0);
  for (int p = 0; p < P; p++)
    for (int c = 0; c < nplan; c++) {
      const int g1 = e->ct_g1[p], g2 = e->ct_g2[p];
      const bool a1 = above(c, g1), a2 = above(c, g2);
      if (a1 != a2) W[(size_t)p * nplan + c] = lever(a1 ? g1 : g2, c);
    }
  return W;
}

// ---- chain program shared by the pose and IK handles: per body {njnt}, per joint {type, qadr, jid}
int build_chain(const HostModel &m, int site_body, std::vector<int> &pi, std::vector<double> &pd, int *nj) {
  std::vector<int> chain;
  for (int b = site_body; b > 0; b = m.body_parentid[b]) chain.push_back(b);
  std::reverse(chain.begin(), chain.end());
  pi.assign(PH_SIZE, 0);
  *nj = 0;
  for (int b : chain) {
    pi.push_back(m.body_jntnum[b]);
    for (int k = 0; k < 3; k++) pd.push_back(m.body_pos[3 * b + k]);
    for (int k = 0; k < 4; k++) pd.push_back(m.body_quat[4 * b + k]);
    for (int j = 0; j < m.body_jntnum[b]; j++) {
      const int jid = m.body_jntadr[b] + j;
      if (m.jnt_type[jid] != JT_SLIDE && m.jnt_type[jid] != JT_HINGE)
        return fail(MJPL_E_JOINT, "joint %d: only slide and hinge joints are supported", jid);
      pi.push_back(m.jnt_type[jid]);
      pi.push_back(m.jnt_qposadr[jid]);
      pi.push_back(jid);
      for (int k = 0; k < 3; k++) pd.push_back(m.jnt_axis[3 * jid + k]);
      for (int k = 0; k < 3; k++) pd.push_back(m.jnt_pos[3 * jid + k]);
      pd.push_back(m.qpos0[m.jnt_qposadr[jid]]);
      (*nj)++;
    }
  }
  pi[PH_NBODY] = (int)chain.size();
  pi[PH_NJOINT] = *nj;
  pi[PH_NQ] = m.nq;
  return MJPL_OK;
}

// what a generated projection carries as literals: the chain program without its run-time tail (site offset,
// constraint, tolerances, iteration bound), the library ABI and the digest of the shared headers
uint64_t chain_hash_of(const std::vector<int> &pi, const std::vector<double> &pd, size_t chain_doubles) {
  Fnv1a f;
  const int head[3] = {pi[PH_NBODY], pi[PH_NJOINT], pi[PH_NQ]};
  f.mix(head, sizeof(head));
  f.mix(pi.data() + PH_SIZE, (pi.size() - PH_SIZE) * sizeof(int));
  f.mix(pd.data(), chain_doubles * sizeof(double));
  f.mixi(MJPL_SPEC_ABI);
  f.mix_stamp();
  return f.h;
}

}  // namespace
