// mjpl_contacts.h -- which candidate geom pairs touch, per configuration (mjpl_contacts*).
//
// What it replaces: the contact list `data.contact.geom` that CollisionConstraint.valid_config
// reads after mj_kinematics + mj_collision (reference src/mjpl/constraint/collision_constraint.py:26-30)
// and hands to CollisionRuleset.obeys_ruleset (:66-95).  The check kernels fold the ruleset into
// their pair list and stop at a configuration's first contact; this kernel decides EVERY candidate
// pair of mj_collision, allowed pairs included, and reports one bit per pair.
//
// Shape: one lane per configuration.
//   1. The lane runs the interpreter's float64 forward kinematics (run_config with EMIT, the walk the
//      FK parity kernel k_fk runs) and writes its moving geoms' world poses into a scratch row.
//   2. It walks the candidate table in the oracle's order (g1 < g2, g1 outer).  The pair index is
//      wave-uniform, so the branch on the pair's types is uniform too.  Per pair: the bound cull of
//      the check (mj_collideSphere / the plane cull), then -- if any lane of the wave passed it --
//      the check's own float64 narrowphase (pair_contact), with the check's argument order, margin
//      and bound.  A pair's bit is therefore the per-pair decision the check makes.
//   3. Bits are gathered into a 64-bit register word and stored once per word: word w of
//      configuration i goes to bits[i * W + w].
// Static partners come from the engine's world tables (cull table: position; narrow table: axes and
// size), the same rows the check reads.  No float32 filter runs in front of this path.
#pragma once

namespace mjpl {

// candidate table, one record per pair (built at mjpl_create, mjpl_compile.h: build_contact_table).
// `cur` is the moving geom the check places LATER (its partner `par` is a static geom or an earlier
// moving one), exactly as run_config pairs them.
enum : int { CI_CUR = 0,  // model geom id of cur (moving)
             CI_PAR,      // model geom id of par (moving), or its world-table row (static: CF_STATIC)
             CI_TCUR, CI_TPAR, CI_FLAGS, CI_PARID, CI_LEN = 8 };
enum : int { CF_PFIRST = 1,   // par is g1 of mj_collision's type-ordered pair (pair_contact's `pfirst`)
             CF_STATIC = 2 }; // par is welded to the world: read from the world tables
// doubles: pair margin max(m1, m2); cull bound ((r1 + r2 + margin)^2, margin + rbound for a plane,
// +inf where mj_collision has no bound test); cur's size
enum : int { CD_MARGIN = 0, CD_BOUND, CD_SCUR, CD_SPAR = 5, CD_LEN = 8 };

// configurations per launch: the FK scratch holds one row of ngeom poses per configuration
constexpr int64_t kContactRows = (int64_t)1 << 16;

// world pose of a moving geom from this lane's scratch row; only the z axis unless it is a box
__device__ __forceinline__ void contact_load_geom(GeomT<double> &g, const double *gx, const double *gm, int geom,
                                                  int type) {
#pragma unroll
  for (int k = 0; k < 3; k++) g.pos[k] = gx[3 * geom + k];
  if (type == GT_BOX) {
#pragma unroll
    for (int k = 0; k < 9; k++) g.m[k] = gm[9 * geom + k];
  } else {
    g.m[0] = g.m[1] = g.m[3] = g.m[4] = g.m[6] = g.m[7] = 0;
    g.m[2] = gm[9 * geom + 2]; g.m[5] = gm[9 * geom + 5]; g.m[8] = gm[9 * geom + 8];
  }
}

// Candidate pair p, its geoms placed as the check places them: cur from the lane's scratch row, par from it (moving)
// or from the world tables (static: cull table position, narrow table axes and size).  Inactive lanes get zero poses.
// UNI: p is wave-uniform and the record is read as such (the walks); the epilogue's p differs per lane.
struct PairGeoms {
  int gcur, gparid, tcur, tpar, flags;  // model geom ids of cur and par, CI_TCUR, CI_TPAR, CI_FLAGS
  GeomT<double> cur, par;
  double scur[3], spar[3];
};

template <bool UNI>
__device__ __forceinline__ PairGeoms contact_load_pair(IP ct, DP cd, int p, const double *rx, const double *rm,
                                                       DP wcull, DP wnarrow, bool active) {
  IP e = ct + p * CI_LEN;
  DP d = cd + p * CD_LEN;
  auto rec = [](int v) { return UNI ? uni(v) : v; };
  PairGeoms g;
  const int gpar = rec(e[CI_PAR]);
  g.gcur = rec(e[CI_CUR]);
  g.gparid = rec(e[CI_PARID]);
  g.tcur = rec(e[CI_TCUR]);
  g.tpar = rec(e[CI_TPAR]);
  g.flags = rec(e[CI_FLAGS]);
  for (int k = 0; k < 3; k++) g.scur[k] = d[CD_SCUR + k];
  if (active) contact_load_geom(g.cur, rx, rm, g.gcur, g.tcur);
  else g.cur = GeomT<double>{};
  if (g.flags & CF_STATIC) {
    DP rw = wnarrow + gpar * WN_LEN;
    g.par.pos[0] = wcull[wc_at(gpar, 0)]; g.par.pos[1] = wcull[wc_at(gpar, 1)]; g.par.pos[2] = wcull[wc_at(gpar, 2)];
    g.par.m[2] = rw[WN_ZAXIS]; g.par.m[5] = rw[WN_ZAXIS + 1]; g.par.m[8] = rw[WN_ZAXIS + 2];
    g.par.m[0] = rw[WN_XAXIS]; g.par.m[3] = rw[WN_XAXIS + 1]; g.par.m[6] = rw[WN_XAXIS + 2];
    g.par.m[1] = rw[WN_YAXIS]; g.par.m[4] = rw[WN_YAXIS + 1]; g.par.m[7] = rw[WN_YAXIS + 2];
    // (a plane's narrowphase size is no input of the plane routines; the check passes zeros)
    for (int k = 0; k < 3; k++) g.spar[k] = g.tpar == GT_PLANE ? 0.0 : rw[WN_SIZE + k];
  } else {
    if (active) contact_load_geom(g.par, rx, rm, gpar, g.tpar);
    else g.par = GeomT<double>{};
    for (int k = 0; k < 3; k++) g.spar[k] = d[CD_SPAR + k];
  }
  return g;
}

// Configurations [i0, i0 + n) of the batch Q (N rows, `layout`); scratch row r = i - i0 holds
// configuration i's moving geom poses: gx [n][ngeom][3], gm [n][ngeom][9].
__global__ void __launch_bounds__(kBlock)
k_contacts(const int *__restrict__ gip, int nip, const double *__restrict__ gdp, int ndp,
           const int *__restrict__ gct, const double *__restrict__ gcd, int P, int W,
           const double *__restrict__ Q, int64_t N, int64_t i0, int64_t n, int layout,
           double *__restrict__ gx, double *__restrict__ gm, int ngeom, unsigned long long *__restrict__ bits) {
  extern __shared__ double smem[];
  const int B = blockDim.x;
  const int nplan = gip[H_NPLAN];
  Carve<double> c = carve_lds<double>(smem, gip, nip, gdp, ndp, nplan, 1, B);
  const int64_t r = (int64_t)blockIdx.x * B + threadIdx.x;
  const bool active = r < n;
  const int64_t i = i0 + (active ? r : 0);
  load_columns(c.col0 + threadIdx.x, B, Q, N, i, nplan, layout, active);
  __syncthreads();

  // 1. forward kinematics into the scratch row (inactive lanes walk along and write nothing)
  FkOut out = {};
  out.geom_xpos = gx;
  out.geom_xmat = gm;
  out.ngeom = ngeom;
  run_config<double, 1, true, true, true>(c.ip, c.tp, c.col0 + threadIdx.x, B, c.save + threadIdx.x, B, active, 0.0,
                                          out, active ? r : 0);
  const double *rx = gx + (active ? r : 0) * ngeom * 3;
  const double *rm = gm + (active ? r : 0) * ngeom * 9;

  // 2. every candidate pair, in table order
  IP ct = (IP)gct;
  DP cd = (DP)gcd;
  DP wcull = c.tp + uni(c.ip[H_OFF_WCULL]);
  DP wnarrow = c.tp + uni(c.ip[H_OFF_WNARROW]);
  for (int w = 0; w < W; w++) {
    unsigned long long word = 0;
    const int pend = P < 64 * (w + 1) ? P : 64 * (w + 1);
    for (int p = 64 * w; p < pend; p++) {
      const PairGeoms g = contact_load_pair<true>(ct, cd, p, rx, rm, wcull, wnarrow, active);
      DP d = cd + p * CD_LEN;
      // the check's bound cull: plane partners by signed distance, all others by centre distance
      const double bound = d[CD_BOUND];
      bool pass;
      {
        const double dif[3] = {g.cur.pos[0] - g.par.pos[0], g.cur.pos[1] - g.par.pos[1], g.cur.pos[2] - g.par.pos[2]};
        if (g.tpar == GT_PLANE) {
          const double nrm[3] = {g.par.m[2], g.par.m[5], g.par.m[8]};
          pass = !(dot3(dif, nrm) > bound);
        } else {
          pass = !(dif[0] * dif[0] + dif[1] * dif[1] + dif[2] * dif[2] > bound);
        }
      }
      pass = pass && active;
      if (__builtin_amdgcn_ballot_w64(pass) == 0ull) continue;
      const int code = pair_contact<double, true, true>(g.tcur, g.cur, g.scur, g.tpar, g.par, g.spar,
                                                        (g.flags & CF_PFIRST) != 0, d[CD_MARGIN], 0.0);
      if (pass && code == V_CONTACT) word |= 1ull << (p & 63);
    }
    if (active) bits[i * W + w] = word;
  }
}

}  // namespace mjpl
