// mjpl_cplan.h -- batched planning under a PoseConstraint (mjpl_plan_paths_constrained*, include/mjpl_hip.h).
//
// What it adds to mjpl_plan.h: every tree edge is ONE projected step of at most epsilon (cstep: step, the projection
// pose_project_lane with q_old = the node stepped from, the three rules of the reference's _constrained_extend), an
// extension candidate is a chain of up to `extend` such steps (mjpl_plan_paths_constrained_ext*; 1 = a single step), and
// the two trees are joined by a bridge -- a chain of up to `chain` projected steps from the growing tree towards the closest
// of the nodes the other tree gained, closed by one straight edge of at most epsilon -- instead of one straight connect
// edge of any length, whose interior would leave the constraint manifold.  A chain is generated before any verdict is
// known: a projected step depends on the projected row before it, not on that row's collision verdict (the argument of
// k_rrt_gen_project, mjpl_project.h), so links, closing edge and extensions of every problem still go to ONE launch of
// the edge pipeline per round.  tests/cplan_reference.py (extend = 1) and tests/cplan_extend_reference.py are the NumPy
// statement, operation for operation; DESIGN.md 5.18 has the reasoning.  All float64, -ffp-contract=off; integer atomics
// on the round's header only.
//
// Kernels, in launch order (one wave per problem unless said otherwise; no workgroup barrier anywhere):
//   k_cplan_init     the NaN / inf scan, the roots, the ends as planning rows (configuration launch) and as full qpos
//                    rows (mjpl_pose_valid), the counters.
//   (launch_configs and k_pose_valid: the ends' verdicts)
//   k_cplan_propose  round 0: an invalid end retires the problem.  A full growing tree retires it (NODES).  The bridge
//                    pair by a (d2, p) minimum over the wave; lane l draws extension target l and finds its nearest node.
//   k_cplan_project  ONE LANE per row, 64 to a workgroup, LDS per lane qw[nq] | jst[6 njoint] | qo[nq] | t[nplan].  The
//                    first ceil(nb / 64) workgroups take a problem's bridge chain per lane, its steps in sequence; the
//                    others take one extension candidate per lane, up to `extend` steps in sequence -- so a wave's lanes
//                    all run chains of one kind, and it leaves its loop when none of them is going.  Bridge links, the
//                    extension chains' links and their counts.
//   k_cplan_count    the problem's edges: links + closing edge + every link of the extension chains that still fit (an
//                    integer prefix sum over the wave's per-lane link counts); the header
//                    (edges: sum, longest edge: max of the bits of a non-negative double, problems at work: count).
//   (rocprim::exclusive_scan of the per-problem counts)
//   k_cplan_gather   the problem's edges into the AoS edge batch: links, closing edge, chain l's links at the prefix of l.
//   (launch_edges: the verdicts)
//   k_cplan_commit   the leading valid links appended (a ballot); all links and the closing edge valid: SOLVED, the
//                    junctions kept; otherwise each chain's leading valid links appended at the prefix over the lanes
//                    before it, cut where the tree is full.
//   k_cplan_finish   the parent walks into P, LONG for a path of more than max_rows rows, status and counters.
#pragma once

#include "mjpl_plan.h"     // PlanBatch, plan_d2, plan_nearest, plan_problem, plan_tree
#include "mjpl_project.h"  // pose_project_lane, kPoseBlock, kRrtMaxPlan

namespace mjpl {

constexpr int kPlanLong = 5;         // MJPL_PLAN_LONG
constexpr int kCplanMaxChain = 32;   // links of a bridge: a lane of the ballot each, the closing edge after them

constexpr int kCplanMaxExtend = 32;  // links of an extension chain: K X <= 2048 edges beside the bridge's

// PlanBatch's members keep their meaning (P has max_rows rows per problem, not R + 2); conn [nb][3] holds the bridge:
// has a closing edge, its node p of the other tree, the node n of the growing tree the chain starts from.
struct CplanBatch : PlanBatch {
  int S, X, max_rows;  // chain, extend, rows of P per problem
  // the projection: the handle's chain program, the planning columns and their inverse (-1: not a planning column)
  const int *pi;
  const double *pd;
  const int *qidx, *qinv;
  const double *qbase;
  int nq;
  double *cy;      // [nb][X][d][64]: the links of the round's extension chains
  int *cn;         // [nb][64]: the links of candidate l's chain (0: its first step was void)
  double *cl;      // [nb][S][d]: the round's links
  int *nlinks;     // [nb]
  double *cfq;     // [2 nb][nq]: the ends as full rows
  const uint8_t *pvalid;
};

__global__ void __launch_bounds__(64 * kPlanWaves) k_cplan_init(CplanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const double *qi = a.QI + (int64_t)(a.b0 + p) * a.d, *qg = a.QG + (int64_t)(a.b0 + p) * a.d;
  bool bad = false;
  for (int c = lane; c < a.d; c += 64) bad |= !isfinite(qi[c]) || !isfinite(qg[c]);
  const bool any_bad = __ballot(bad) != 0ull;
  double *t0 = plan_tree(a, p, 0), *t1 = plan_tree(a, p, 1), *cf = a.cfg + (int64_t)p * 2 * a.d;
  for (int c = lane; c < a.d; c += 64) {
    t0[c] = qi[c];
    t1[c] = qg[c];
    cf[c] = any_bad ? 0.0 : qi[c];
    cf[a.d + c] = any_bad ? 0.0 : qg[c];
  }
  double *fq = a.cfq + (int64_t)p * 2 * a.nq;
  for (int k = lane; k < a.nq; k += 64) {
    const int c = a.qinv[k];
    fq[k] = c < 0 ? a.qbase[k] : (any_bad ? 0.0 : qi[c]);
    fq[a.nq + k] = c < 0 ? a.qbase[k] : (any_bad ? 0.0 : qg[c]);
  }
  if (lane == 0) {
    a.par[((int64_t)p * 2 + 0) * a.N] = -1;
    a.par[((int64_t)p * 2 + 1) * a.N] = -1;
    a.n[p * 2] = a.n[p * 2 + 1] = 1;
    a.state[p] = any_bad ? kPlanNonFinite : kPlanActive;
    a.gained[p] = 0;
    a.rused[p] = 0;
    a.nedges[p] = 0;
    a.nlinks[p] = 0;
    a.conn[p * 3] = 0;
    a.jn[p * 2] = a.jn[p * 2 + 1] = 0;
    a.cnt[p] = 0;
    if (p == 0) a.cnt[a.nb] = 0;
  }
}

__global__ void __launch_bounds__(64 * kPlanWaves) k_cplan_propose(CplanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  int st = a.state[p];
  const int r = a.round, g = r & 1, o = 1 - g;
  const int ng = a.n[p * 2 + g], no = a.n[p * 2 + o];
  if (st == kPlanActive) {
    if (r == 0 && !(a.cvalid[p * 2] && a.cvalid[p * 2 + 1] && a.pvalid[p * 2] && a.pvalid[p * 2 + 1])) st = kPlanInvalidEnd;
    else if (ng >= a.N) st = kPlanNodes;
    if (st != kPlanActive && lane == 0) {
      a.state[p] = st;
      a.rused[p] = r;
    }
  }
  if (st != kPlanActive) return;
  const int d = a.d;
  const double *Tg = plan_tree(a, p, g), *To = plan_tree(a, p, o);
  // the bridge target: candidate q is the q-th of the last m nodes of the other tree; the least d2 wins, ties to the lowest q
  // (m = the nodes that tree gained in its round, at most S + 64 X = 2080 and less than its size: the scan strides over them)
  const int gained = a.gained[p], m = gained > 1 ? gained : 1;
  double mb = 0.0;
  int mq = -1, mn = 0;
  for (int q = lane; q < m; q += 64) {
    double v;
    const int n = plan_nearest(Tg, ng, To + (int64_t)(no - m + q) * d, 1, d, &v);
    if (mq < 0 || v < mb) {
      mb = v;
      mq = q;
      mn = n;
    }
  }
  for (int w = 32; w > 0; w >>= 1) {
    const double ob = __shfl_xor(mb, w);
    const int oq = __shfl_xor(mq, w), on = __shfl_xor(mn, w);
    if (oq >= 0 && (mq < 0 || ob < mb || (ob == mb && oq < mq))) {
      mb = ob;
      mq = oq;
      mn = on;
    }
  }
  if (lane == 0) {
    a.conn[p * 3 + 1] = no - m + mq;
    a.conn[p * 3 + 2] = mn;
  }
  // the extensions' targets and the nodes they step from
  const int room = a.N - ng, next = a.K < room ? a.K : room;
  if (lane < next) {
    double *t = a.ct + (int64_t)p * d * 64 + lane;
    unsigned long long z = shortcut_mix(shortcut_mix(a.seed_mixed ^ (unsigned long long)(a.b0 + p)) ^ (64ull * (unsigned long long)r + (unsigned long long)lane));
    for (int c = 0; c < d; c++) {
      const double u = (double)(z >> 11) * 0x1.0p-53;
      const double lo = a.box[c], w = a.box[d + c] - lo;
      t[c * 64] = lo + u * w;
      z = shortcut_mix(z);
    }
    double best;
    a.ck[p * 64 + lane] = plan_nearest(Tg, ng, t, 64, d, &best);
  }
}

// cstep(a, t) of one lane: qo holds a as a full row, tt the target (both at a stride of kPoseBlock, LDS); qw receives
// step(a, t), then its projection.  Every lane of the wave calls it (`going` false: the lane only keeps company).
// -> the result is not void; y is then the planning columns of qw.
__device__ __forceinline__ bool cplan_cstep(const CplanBatch &a, double *qw, double *jst, const double *qo, const double *tt, bool going) {
  constexpr int B = kPoseBlock;
  const int d = a.d, nq = a.nq;
  double dat = 0.0;  // d2(a, t)
  if (going) {
    for (int c = 0; c < d; c++) {
      const double v = tt[c * B] - qo[a.qidx[c] * B];
      dat += v * v;
    }
    const double m = sqrt(dat);
    for (int k = 0; k < nq; k++) qw[k * B] = qo[k * B];
    for (int c = 0; c < d; c++) {
      const double av = qo[a.qidx[c] * B], tv = tt[c * B];
      qw[a.qidx[c] * B] = m <= a.epsilon ? tv : av + ((tv - av) / m) * a.epsilon;
    }
  }
  int it = 0;
  const int result = pose_project_lane(a.pi, a.pd, qw, jst, qo, B, going, &it);
  if (!going) return false;
  bool ok = result == 1;
  for (int k = 0; k < nq; k++)  // a projection that moves a joint outside the planning set is refused
    if (a.qinv[k] < 0) ok = ok && __double_as_longlong(qw[k * B]) == __double_as_longlong(a.qbase[k]);
  double day = 0.0, dyt = 0.0;  // d2(a, y), d2(y, t)
  for (int c = 0; c < d; c++) {
    const double y = qw[a.qidx[c] * B];
    const double v = y - qo[a.qidx[c] * B], u = tt[c * B] - y;
    day += v * v;
    dyt += u * u;
  }
  return ok && !(sqrt(day) < 1e-8) && !(dyt > dat);
}

// chain_blocks = ceil(nb / 64) workgroups of bridge chains (lane = problem, up to S steps in sequence), then
// ceil(nb K / 64) of extension candidates (lane = candidate, up to X steps in sequence): one loop, left when no lane of
// the wave is going, so the projection is inlined once
__global__ void __launch_bounds__(kPoseBlock) k_cplan_project(CplanBatch a, int chain_blocks) {
  extern __shared__ double smem[];
  constexpr int B = kPoseBlock;
  const int lane = threadIdx.x, d = a.d, nq = a.nq, nj = a.pi[PH_NJOINT];
  const int g = a.round & 1, o = 1 - g;
  double *qw = smem + lane;
  double *jst = smem + (size_t)nq * B + lane;
  double *qo = smem + ((size_t)nq + 6 * (size_t)nj) * B + lane;
  double *tt = smem + (2 * (size_t)nq + 6 * (size_t)nj) * B + lane;
  const bool is_chain = (int)blockIdx.x < chain_blocks;  // (the same for every lane of the workgroup)
  int p, l = 0;
  if (is_chain) {
    p = blockIdx.x * B + lane;
  } else {
    const int64_t i = (int64_t)((int)blockIdx.x - chain_blocks) * B + lane;
    p = (int)(i / a.K);
    l = (int)(i - (int64_t)p * a.K);
  }
  bool going = p < a.nb && a.state[p] == kPlanActive;
  int budget = 1;
  if (going) {
    const int room = a.N - a.n[p * 2 + g];
    if (is_chain) budget = a.S < room ? a.S : room;
    else going = l < (a.K < room ? a.K : room);
  }
  if (__ballot(going) == 0ull) return;
  if (going) {
    const double *Tg = plan_tree(a, p, g);
    const double *from = Tg + (int64_t)(is_chain ? a.conn[p * 3 + 2] : a.ck[p * 64 + l]) * d;
    const double *t = is_chain ? plan_tree(a, p, o) + (int64_t)a.conn[p * 3 + 1] * d : a.ct + (int64_t)p * d * 64 + l;
    const int ts = is_chain ? 1 : 64;
    for (int k = 0; k < nq; k++) qo[k * B] = a.qbase[k];
    for (int c = 0; c < d; c++) {
      qo[a.qidx[c] * B] = from[c];
      tt[c * B] = t[c * ts];
    }
  }
  const bool mine = going;
  const int steps = is_chain ? a.S : a.X;
  // where this lane's links go: a bridge's rows are contiguous, an extension chain's lane-minor
  double *const out = is_chain ? a.cl + (int64_t)p * a.S * d : a.cy + (int64_t)p * a.X * d * 64 + l;
  const int os = is_chain ? 1 : 64;
  int links = 0, closing = 0;
  for (int s = 0; s < steps && __ballot(going) != 0ull; s++) {
    if (going && is_chain) {
      if (s >= budget) {
        going = false;
      } else {
        double dd = 0.0;
        for (int c = 0; c < d; c++) {
          const double v = tt[c * B] - qo[a.qidx[c] * B];
          dd += v * v;
        }
        if (sqrt(dd) <= a.epsilon) {  // the closing edge: c_{s-1} -> t
          closing = 1;
          going = false;
        }
      }
    }
    const bool good = cplan_cstep(a, qw, jst, qo, tt, going);
    if (going) {
      if (good) {  // a link; the next step is taken from it
        double *y = out + (int64_t)links * d * os;
        for (int c = 0; c < d; c++) y[c * os] = qw[a.qidx[c] * B];
        for (int k = 0; k < nq; k++) qo[k * B] = qw[k * B];
        links++;
      } else {
        going = false;
      }
    }
  }
  if (mine) {
    if (is_chain) {
      a.nlinks[p] = links;
      a.conn[p * 3] = closing;
    } else {
      a.cn[p * 64 + l] = links;
    }
  }
}

// the links of lane l's extension chain, 0 for a chain that does not fit beside the round's links: lanes
// l < min(K, N - n_g - links) count
__device__ __forceinline__ int cplan_ext(const CplanBatch &a, int p, int lane, int ng, int links) {
  const int room = a.N - ng - links, next = a.K < room ? a.K : room;
  return lane < next ? a.cn[p * 64 + lane] : 0;
}

// plan_d2 of two lane-minor rows (both at a stride of 64)
__device__ __forceinline__ double cplan_d2_lanes(const double *a, const double *t, int d) {
  double s = 0.0;
  for (int c = 0; c < d; c++) {
    const double v = t[c * 64] - a[c * 64];
    s += v * v;
  }
  return s;
}

// the sum of v over the lanes below this one, and over the wave (every lane of the wave calls it)
__device__ __forceinline__ int cplan_prefix(int v, int lane, int *total) {
  int incl = v;
  for (int w = 1; w < 64; w <<= 1) {
    const int below = __shfl_up(incl, w);
    if (lane >= w) incl += below;
  }
  *total = __shfl(incl, 63);
  return incl - v;
}

__global__ void __launch_bounds__(64 * kPlanWaves) k_cplan_count(CplanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  if (a.state[p] != kPlanActive) {
    if (lane == 0) a.cnt[p] = 0;
    return;
  }
  const int d = a.d, g = a.round & 1, o = 1 - g, ng = a.n[p * 2 + g];
  const int links = a.nlinks[p], closing = a.conn[p * 3];
  const double *Tg = plan_tree(a, p, g), *cl = a.cl + (int64_t)p * a.S * d;
  const double *first = Tg + (int64_t)a.conn[p * 3 + 2] * d;
  const int ext = cplan_ext(a, p, lane, ng, links);
  int exts;
  cplan_prefix(ext, lane, &exts);
  const int count = links + closing + exts;
  // the longest edge: lane s < links holds link s, lane `links` the closing edge; every lane the links of its chain
  double longest = 0.0;
  if (lane < links + closing) {
    const double *qa = lane == 0 ? first : cl + (int64_t)(lane - 1) * d;
    const double *qb = lane < links ? cl + (int64_t)lane * d : plan_tree(a, p, o) + (int64_t)a.conn[p * 3 + 1] * d;
    longest = sqrt(plan_d2(qa, qb, 1, d));
  }
  const double *cy = a.cy + (int64_t)p * a.X * d * 64 + lane;
  for (int s = 0; s < ext; s++) {
    const double *y = cy + (int64_t)s * d * 64;
    const double len = s == 0 ? sqrt(plan_d2(Tg + (int64_t)a.ck[p * 64 + lane] * d, y, 64, d)) : sqrt(cplan_d2_lanes(y - (int64_t)d * 64, y, d));
    if (len > longest) longest = len;  // (NaN never compares greater)
  }
  for (int w = 32; w > 0; w >>= 1) {
    const double other = __shfl_xor(longest, w);
    if (other > longest) longest = other;
  }
  if (lane == 0) {
    a.cnt[p] = count;
    a.nedges[p] += count;
    atomicMax(&a.head[0], (unsigned long long)__double_as_longlong(longest));
    atomicAdd(&a.head[1], (unsigned long long)count);
    atomicAdd(&a.head[2], 1ull);
  }
}

__global__ void __launch_bounds__(64 * kPlanWaves) k_cplan_gather(CplanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const int cnt = a.cnt[p];
  if (cnt == 0) return;
  const int d = a.d, g = a.round & 1, o = 1 - g, ng = a.n[p * 2 + g];
  const int links = a.nlinks[p], closing = a.conn[p * 3];
  const double *Tg = plan_tree(a, p, g), *cl = a.cl + (int64_t)p * a.S * d;
  const double *first = Tg + (int64_t)a.conn[p * 3 + 2] * d, *target = plan_tree(a, p, o) + (int64_t)a.conn[p * 3 + 1] * d;
  const int64_t e0 = (int64_t)a.off[p] * d;  // (off[p] + cnt <= nb (S + 1 + K X): the batch is sized for that)
  for (int i = lane; i < (links + closing) * d; i += 64) {
    const int j = i / d, c = i - j * d;
    a.QA[e0 + i] = j == 0 ? first[c] : cl[(int64_t)(j - 1) * d + c];
    a.QB[e0 + i] = j < links ? cl[(int64_t)j * d + c] : target[c];
  }
  const int ext = cplan_ext(a, p, lane, ng, links);
  int exts;
  const int before = cplan_prefix(ext, lane, &exts);
  const double *from = Tg + (int64_t)a.ck[p * 64 + lane] * d, *cy = a.cy + (int64_t)p * a.X * d * 64 + lane;
  for (int s = 0; s < ext; s++) {  // chain `lane`: link s runs from link s - 1 (the nearest node for s = 0)
    const int64_t e = e0 + (int64_t)(links + closing + before + s) * d;
    const double *y = cy + (int64_t)s * d * 64;
    for (int c = 0; c < d; c++) {
      a.QA[e + c] = s == 0 ? from[c] : y[(c - d) * 64];
      a.QB[e + c] = y[c * 64];
    }
  }
}

__global__ void __launch_bounds__(64 * kPlanWaves) k_cplan_commit(CplanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0 || a.state[p] != kPlanActive) return;
  const int d = a.d, r = a.round, g = r & 1, o = 1 - g, ng = a.n[p * 2 + g];
  const int links = a.nlinks[p], closing = a.conn[p * 3];
  const int64_t e0 = a.off[p];  // (read only where the problem has an edge: cnt > 0)
  double *Tg = plan_tree(a, p, g);
  int *par = a.par + ((int64_t)p * 2 + g) * a.N;
  // the leading valid links (links <= 32 <= N - n_g)
  const unsigned long long bad = __ballot(lane < links && a.valid[e0 + lane] == 0);
  const int first_bad = bad ? __ffsll((long long)bad) - 1 : links, lead = first_bad < links ? first_bad : links;
  if (lane < lead) {
    const double *y = a.cl + ((int64_t)p * a.S + lane) * d;
    for (int c = 0; c < d; c++) Tg[(int64_t)(ng + lane) * d + c] = y[c];
    par[ng + lane] = lane == 0 ? a.conn[p * 3 + 2] : ng + lane - 1;
  }
  if (closing && lead == links && a.valid[e0 + links] != 0) {
    if (lane == 0) {
      a.state[p] = kPlanSolved;
      a.rused[p] = r + 1;
      a.jn[p * 2 + g] = links > 0 ? ng + links - 1 : a.conn[p * 3 + 2];
      a.jn[p * 2 + o] = a.conn[p * 3 + 1];
      a.n[p * 2 + g] = ng + lead;
      a.gained[p] = lead;
    }
    return;
  }
  // the extension chains: lane l's leading valid links, appended after those of the lanes below it, as many as fit
  const int ext = cplan_ext(a, p, lane, ng, links);
  int exts, oks;
  const int64_t ve = e0 + links + closing + cplan_prefix(ext, lane, &exts);
  int ok = 0;
  while (ok < ext && a.valid[ve + ok] != 0) ok++;
  const int below = cplan_prefix(ok, lane, &oks);
  const int room = a.N - ng - lead;  // (>= 0: lead <= links <= N - n_g)
  const int start = below < room ? below : room, take = ok < room - start ? ok : room - start;
  const int at = ng + lead + start;  // (at + take <= N)
  const double *cy = a.cy + (int64_t)p * a.X * d * 64 + lane;
  for (int s = 0; s < take; s++) {
    const double *y = cy + (int64_t)s * d * 64;
    for (int c = 0; c < d; c++) Tg[(int64_t)(at + s) * d + c] = y[c * 64];
    par[at + s] = s == 0 ? a.ck[p * 64 + lane] : at + s - 1;
  }
  if (lane == 0) {
    const int got = oks < room ? oks : room;
    a.n[p * 2 + g] = ng + lead + got;
    a.gained[p] = lead + got;
  }
}

// (P arrives zeroed)
__global__ void __launch_bounds__(64 * kPlanWaves) k_cplan_finish(CplanBatch a) {
  const int p = plan_problem(a), lane = threadIdx.x & 63;
  if (p < 0) return;
  const int b = a.b0 + p, d = a.d;
  int st = a.state[p];
  int rows = 0;
  if (st == kPlanSolved) {
    const double *T0 = plan_tree(a, p, 0), *T1 = plan_tree(a, p, 1);
    const int *par0 = a.par + ((int64_t)p * 2 + 0) * a.N, *par1 = a.par + ((int64_t)p * 2 + 1) * a.N;
    double *P = a.P + (int64_t)b * a.max_rows * d;
    // (a chain of parents is at most N long: the guards keep a broken one finite)
    int len0 = 0, len1 = 0;
    for (int k = a.jn[p * 2]; k >= 0 && len0 < a.N; k = par0[k]) len0++;
    for (int k = a.jn[p * 2 + 1]; k >= 0 && len1 < a.N; k = par1[k]) len1++;
    if (len0 + len1 > a.max_rows) {
      st = kPlanLong;
    } else {
      int i = len0 - 1;
      for (int k = a.jn[p * 2]; k >= 0 && i >= 0; k = par0[k], i--)
        for (int c = lane; c < d; c += 64) P[(int64_t)i * d + c] = T0[(int64_t)k * d + c];
      rows = len0;
      for (int k = a.jn[p * 2 + 1]; k >= 0 && rows < len0 + len1; k = par1[k], rows++)
        for (int c = lane; c < d; c += 64) P[(int64_t)rows * d + c] = T1[(int64_t)k * d + c];
    }
  }
  if (lane == 0) {
    const bool grew = st != kPlanNonFinite && st != kPlanInvalidEnd;
    a.n_out[b] = rows;
    a.status[b] = st == kPlanActive ? kPlanRounds : st;
    if (a.rounds_used) a.rounds_used[b] = st == kPlanActive ? a.R : a.rused[p];
    if (a.edges) a.edges[b] = a.nedges[p];
    if (a.tree_nodes) {
      a.tree_nodes[(int64_t)b * 2] = grew ? a.n[p * 2] : 0;
      a.tree_nodes[(int64_t)b * 2 + 1] = grew ? a.n[p * 2 + 1] : 0;
    }
  }
}

}  // namespace mjpl
