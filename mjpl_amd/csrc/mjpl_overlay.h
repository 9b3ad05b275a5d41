// mjpl_overlay.h -- specialisations laid over mjpl_device.h by a forced include (-include) on the hipcc lines of
// mjpl_amd/build.py and mjpl_amd/specialise.py.  NOT one of build.STAMPED_HEADERS: nothing here changes a layout, a
// table or a value, so a library built without this file computes the same results (it is slower, not wrong), and the
// source stamp and the program hashes stay what they are.
//
// slot_get6<float, MAXS> with a run-time slot, MAXS = 4 and 8.  The slot is wave-uniform, but for a vector of up to
// eight elements the compiler expands `v[slot]` into a compare per element and a chain of MAXS - 1 selects per value:
// for the eight-wide slot file of the benchmark model 7 s_cmp + 7 s_cselect + 42 v_cndmask to copy six registers, on
// every push of a stored partner (profiles/README.md, "Stored-partner poses without a select chain").  From sixteen
// elements on it uses indexed moves instead (s_set_gpr_idx_on, v_mov, s_set_gpr_idx_off): three instructions a value.
//
// Both widths read the file through a tree of scalar branches over the slot whose leaves read literal elements.  The
// instruction counts below are those of the kernels as both compile lines build them, with build.codegen_flags()
// (-structurizecfg-skip-uniform-regions): the tree stays compares and scalar branches.  Built WITHOUT that option the
// structuriser wraps the leaves in flag moves and extra branches (about 18 scalar instructions and 6 moves on a path),
// and at width 8 the tree then loses to the indexed moves it replaced (profiles/README.md, "Uniform branches stay
// branches", has both measurements).
#pragma once

#include "../../include/mjpl_hip.h"  // (mjpl_device.h reads the layout constants; mjpl_filter.h includes the two in this order)
#include "mjpl_device.h"

namespace mjpl {

// log2(MAXS) compares and branches, then six moves and a branch to the join.  The barrier on each value keeps the
// leaves separate blocks (without it the compiler folds the tree back into the select chain).
template <int LO, int N, int MAXS>
__device__ __forceinline__ void slot_tree6(const SlotFile<float, MAXS> &sf, int slot, float *t6) {
  if constexpr (N == 1) {
#pragma unroll
    for (int k = 0; k < 6; k++) {
      t6[k] = sf.f[k][LO];
      pin(t6[k]);
    }
  } else {
    if (slot < LO + N / 2)
      slot_tree6<LO, N / 2>(sf, slot, t6);
    else
      slot_tree6<LO + N / 2, N / 2>(sf, slot, t6);
  }
}

// Eight wide: 3 s_cmp + 3 s_cbranch + 6 v_mov_b32 + 1 s_branch = 13 instructions between the test for EK_SLOT and the
// push, six of them vector.  The alternative -- two neighbouring vectors of the file read as ONE sixteen-wide vector
// (__builtin_shufflevector), for which the compiler takes its indexed moves -- is 1 s_add + 6 x (s_set_gpr_idx_on,
// v_mov_b32, s_set_gpr_idx_off) = 19 instructions, no branch; it also holds six more VGPRs in the benchmark library's
// filter kernels and five more spilled ones in its k_edges_fused (16 against 11).  Measured on the benchmark, the tree
// is 2 % faster on the line (k_edges_fused 0.150 -> 0.147 ms).
template <>
__device__ __forceinline__ void slot_get6<float, 8>(const SlotFile<float, 8> &sf, int slot, float *t6) {
  slot_tree6<0, 8>(sf, __builtin_amdgcn_readfirstlane(slot), t6);
}

// Four wide: 2 compares and branches and six moves in place of 4 s_cmp + 4 s_cselect + 18 v_cndmask, with the
// registers and the occupancy of the plain build.  Indexed moves need one sixteen-wide tuple of four vectors and one
// of two, which cost 20 more registers and one wave per SIMD of k_filter_endpoints_pw and k_filter_items_pw
// (random_model(1005): 119 -> 139 and 115 -> 135 VGPRs).
template <>
__device__ __forceinline__ void slot_get6<float, 4>(const SlotFile<float, 4> &sf, int slot, float *t6) {
  slot_tree6<0, 4>(sf, __builtin_amdgcn_readfirstlane(slot), t6);
}

// No specialisation for the sixteen-wide file: the compiler's indexed moves are there already, and the tree measured
// worse (random_model(1002), k_edges_fused: 273 -> 290 spilled VGPRs, 53.7 -> 55.3 KB of code, without the option
// above).  Float64 files and the literal slots of moving-box libraries (SpecSlots) are untouched as well.

// ----------------------------------------------------------------------------- queue_drain<float, BOXQ, ALL, false>
// The drain of the binary32 filter without moving boxes: statement for statement that of mjpl_device.h, but for how the
// waypoint of a candidate it cannot decide is rebuilt for the exact re-check.  There ONE lane walks exact_waypoint alone,
// up to kCkptEvery - 1 steps of nplan float64 divisions and a square root each, while the other 63 lanes of its wave
// wait, and every step reads the edge's end again, 2 nplan loads in a chain: about 1 300 of the 4.9 M candidates of a
// benchmark launch, and an eighth of the kernel's time (profiles/README.md, "Hand-offs walked by the wave").  Here the wave walks it together, lane k holding planning column k: a step is one
// division per lane, and the sum under the root is taken in the reference's order from the lanes' squares -- the same
// operations on the same operands in the same order, so the row written is bit for bit exact_waypoint's.  Slot, row,
// edge, index and geom ids in the undecided list are what they were.
// The timing-only builds of the primary template (MJPL_STAMPS, MJPL_X_NODRAIN, MJPL_X_DRAIN_NONARROW) keep that template.
#if !defined(MJPL_STAMPS) && !defined(MJPL_X_NODRAIN) && !defined(MJPL_X_DRAIN_NONARROW)

__device__ __forceinline__ double lane_value(double x, int l) {  // x of lane l (wave-uniform l)
  const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// exact_waypoint with wave-uniform arguments, called by the lanes 0 .. nplan - 1 at least (nplan <= 64): lane k holds
// out[k].  Every statement of exact_waypoint's recurrence is here once per lane instead of once per column.
__device__ __forceinline__ void exact_waypoint_wave(const EdgeSource &src, IP perm, int nplan, long long i, int idx, double *out,
                                                    long long slot) {
  const int lane = threadIdx.x & 63;
  const bool mine = lane < nplan;
  const int k = mine ? lane : 0;
  auto at = [&](const double *Q) -> double {
    return (src.layout == MJPL_SOA) ? Q[(long long)k * src.E + i] : Q[i * nplan + k];
  };
  int from = 0;
  double o;
  if (src.idx0_end && idx == 0) {
    o = at(src.QB);
  } else if (src.ckpt && slot >= 0 && idx >= kCkptEvery) {
    from = idx - idx % kCkptEvery;
    o = src.ckpt[(size_t)(slot - (idx - from)) * nplan + k];
  } else {
    o = at(src.QA);
  }
  const double b = at(src.QB);
  const int col = perm[k];
  for (int n = from; n < idx; n++) {
    const double d = b - o;
    const double dd = d * d;
    double s = 0;
    for (int c = 0; c < nplan; c++) s = s + lane_value(dd, __builtin_amdgcn_readlane(col, c));
    const double mag = sqrt(s);
    const double sm = src.step < mag ? src.step : mag;
    o = o + (d / mag) * sm;
  }
  if (mine) out[k] = o;
}

template <bool BOXQ, bool ALL>
__device__ __forceinline__ void queue_drain_f32(const WaveQueue<float, false> &wq, int &qn, const float *tp, const float *wcull,
                                                const float *wnarrow, int nwpad, float tol, const PatchSink &ps) {
  typedef const float *Tab;
  typedef GeomT<float> Geom;
  constexpr int CAP = BOXQ ? QB_CAP : QN_CAP;
  const float *qf = BOXQ ? wq.bf : wq.nf;
  const int *qi0 = BOXQ ? wq.bi0 : wq.ni0, *qi1 = BOXQ ? wq.bi1 : wq.ni1;
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  do {  // wave-uniform
    const int n = qn < 64 ? qn : 64;
    const int j = qn - n + lane;
    const bool on = lane < n;
    qn -= n;
    const int jj = on ? j : 0;
    const int i0 = qi0[jj];
    const int i1 = qi1[jj];
    Tab gd = tp + (i1 & 0xffff);
    CertAcc<float> cacc = {0.0f, true};
    cacc.extra = (float)__builtin_bit_cast(_Float16, (unsigned short)((unsigned)i1 >> 16));
    const int owner = i0 & 63, gtype = (i0 >> 6) & 15, ptype = (i0 >> 10) & 15;
    const bool pfirst = (i0 >> 14) & 1;
    const int kind = (i0 >> 15) & 3, index = (i0 >> 17) & 255;
    Geom cur, par;
    cur.pos[0] = qf[0 * CAP + jj]; cur.pos[1] = qf[1 * CAP + jj]; cur.pos[2] = qf[2 * CAP + jj];
    cur.m[2] = qf[3 * CAP + jj]; cur.m[5] = qf[4 * CAP + jj]; cur.m[8] = qf[5 * CAP + jj];
    cur.m[0] = cur.m[1] = cur.m[3] = cur.m[4] = cur.m[6] = cur.m[7] = 0;
    par.m[0] = par.m[1] = par.m[3] = par.m[4] = par.m[6] = par.m[7] = 0;
    const float gsize[3] = {gd[GD_SIZE], gd[GD_SIZE + 1], gd[GD_SIZE + 2]};
    float psize[3], margin;
    int code = V_NONE;
    if constexpr (BOXQ) {
      Tab rw = wnarrow + index * WN_LEN;
      par.pos[0] = wcull[wc_at(index, 0)]; par.pos[1] = wcull[wc_at(index, 1)]; par.pos[2] = wcull[wc_at(index, 2)];
      par.m[2] = rw[WN_ZAXIS]; par.m[5] = rw[WN_ZAXIS + 1]; par.m[8] = rw[WN_ZAXIS + 2];
      par.m[0] = rw[WN_XAXIS]; par.m[3] = rw[WN_XAXIS + 1]; par.m[6] = rw[WN_XAXIS + 2];
      par.m[1] = rw[WN_YAXIS]; par.m[4] = rw[WN_YAXIS + 1]; par.m[7] = rw[WN_YAXIS + 2];
      psize[0] = rw[WN_SIZE]; psize[1] = rw[WN_SIZE + 1]; psize[2] = rw[WN_SIZE + 2];
      margin = gd[GD_WBOUND + nwpad + index];
      if (on) code = pair_contact<float, true, false>(gtype, cur, gsize, GT_BOX, par, psize, pfirst, margin, tol, &cacc);
    } else {
      if (kind == EK_SLOT) {
        par.pos[0] = qf[6 * CAP + jj]; par.pos[1] = qf[7 * CAP + jj]; par.pos[2] = qf[8 * CAP + jj];
        par.m[2] = qf[9 * CAP + jj]; par.m[5] = qf[10 * CAP + jj]; par.m[8] = qf[11 * CAP + jj];
        Tab sb = gd + GD_WBOUND + 2 * nwpad;
        margin = sb[MAX_SLOTS + index];
        psize[0] = sb[2 * MAX_SLOTS + 3 * index]; psize[1] = sb[2 * MAX_SLOTS + 3 * index + 1];
        psize[2] = sb[2 * MAX_SLOTS + 3 * index + 2];
      } else {
        Tab rw = wnarrow + index * WN_LEN;
        par.pos[0] = wcull[wc_at(index, 0)]; par.pos[1] = wcull[wc_at(index, 1)]; par.pos[2] = wcull[wc_at(index, 2)];
        par.m[2] = rw[WN_ZAXIS]; par.m[5] = rw[WN_ZAXIS + 1]; par.m[8] = rw[WN_ZAXIS + 2];
        psize[0] = rw[WN_SIZE]; psize[1] = rw[WN_SIZE + 1]; psize[2] = rw[WN_SIZE + 2];
        margin = gd[GD_WBOUND + nwpad + index];
      }
      if (on) code = pair_contact<float, false, false>(gtype, cur, gsize, ptype, par, psize, pfirst, margin, tol, &cacc);
    }
    if (on && code == V_CONTACT) atomicOr(&wq.flags[owner], 1);
    if (on && cacc.extra > 0.0f && !(code == V_NONE && cacc.clear)) atomicOr(&wq.flags[owner], 4);
    // (an owner known to be in contact needs no exact check of another pair)
    const bool unsure = on && code == V_UNSURE && !(wq.flags[owner] & 1);
#ifndef MJPL_X_NOHANDOFF  // (timing-only build: nothing is handed on and nobody is told)
    // (wave-uniform, and rare: told so, the compiler lays the block out behind the kernel's hot paths)
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(unsure) != 0ull, 0)) {
      // The wave can rebuild a waypoint if the lanes of the planning columns are all here (they are wherever a whole wave
      // checks a tile); where they are not, nothing is handed on and the owners are told so, as when the list is full.
      const unsigned long long cols = ps.nplan >= 64 ? ~0ull : (1ull << ps.nplan) - 1ull;
      const bool can = !ps.src.QA || (ps.nplan <= 64 && (__builtin_amdgcn_ballot_w64(true) & cols) == cols);
      // every lane with such a candidate takes its row of the undecided list and writes what identifies the pair, as ever
      bool handed = false, walk = false;
      int u = 0, item = 0, ed = 0, ix = 0;
      if (unsure && ps.uc.count && can) {
        u = atomicAdd(ps.uc.count, 1);
        if (u < ps.uc.cap) {
          item = (int)((unsigned)wq.flags[owner] >> 3);
          ed = ps.item_edge ? ps.item_edge[item] : item;
          ix = ps.item_idx ? ps.item_idx[item] : ps.idx;
          if (ps.src.QA)  // row `ed` of the caller's configurations (ix = 0), or waypoint ix of edge `ed`: below
            walk = true;
          else
            for (int k = 0; k < ps.nplan; k++) ps.uc.q[(size_t)u * ps.nplan + k] = ps.qcol[k * ps.B + owner * ps.L];
          ps.uc.edge[u] = ed;
          ps.uc.idx[u] = ix;
          ps.uc.ga[u] = (int)gd[GD_GEOMID];
          int gb;
          if (!BOXQ && kind == EK_SLOT) gb = (int)gd[GD_WBOUND + 2 * nwpad + GS_GEOMID + index];
          else gb = info_bits(wcull[wc_at(index, WC_INFO)]) >> 8;
          ps.uc.gb[u] = gb;
          handed = true;
        }
      }
      if (unsure && !handed) atomicOr(&wq.flags[owner], 2);
#ifdef MJPL_X_NOWALK  // timing-only build: rows are taken, their configurations are not written
      walk = false;
#endif
      // ... and the wave rebuilds their waypoints, one after another
      for (unsigned long long m = __builtin_amdgcn_ballot_w64(walk); m; m &= m - 1) {
        const int l = (int)__builtin_ctzll(m);
        const int item_l = __builtin_amdgcn_readlane(item, l);
        exact_waypoint_wave(ps.src, ps.perm, ps.nplan, __builtin_amdgcn_readlane(ed, l), __builtin_amdgcn_readlane(ix, l),
                            ps.uc.q + (size_t)__builtin_amdgcn_readlane(u, l) * ps.nplan, ps.item_idx ? item_l : -1);
      }
    }
#endif
  } while (ALL && qn > 0);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

#define MJPL_OVERLAY_DRAIN(BOXQ, ALL)                                                                                          \
  template <>                                                                                                                  \
  __device__ __forceinline__ void queue_drain<float, BOXQ, ALL, false>(                                                        \
      const WaveQueue<float, false> &wq, int &qn, const float *tp, const float *wcull, const float *wnarrow, int nwpad,       \
      float tol, const PatchSink &ps, unsigned long long *) {                                                                  \
    queue_drain_f32<BOXQ, ALL>(wq, qn, tp, wcull, wnarrow, nwpad, tol, ps);                                                    \
  }
MJPL_OVERLAY_DRAIN(false, false)
MJPL_OVERLAY_DRAIN(false, true)
MJPL_OVERLAY_DRAIN(true, false)
MJPL_OVERLAY_DRAIN(true, true)
#undef MJPL_OVERLAY_DRAIN

#endif  // the timing-only builds of the primary template

}  // namespace mjpl
