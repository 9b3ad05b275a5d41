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

}  // namespace mjpl
