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
#pragma once

#include "../../include/mjpl_hip.h"  // (mjpl_device.h reads the layout constants; mjpl_filter.h includes the two in this order)
#include "mjpl_device.h"

namespace mjpl {

// Eight wide: two neighbouring vectors of the file read as ONE sixteen-wide vector, so that the compiler takes its
// indexed moves: 1 s_add + 6 x 3 instructions, no branch, no select.  The register allocator keeps the pairs
// f[0] f[1], f[2] f[3], f[4] f[5] in adjacent registers for the whole kernel (as it keeps each vector), so the
// concatenation costs no copy -- to be looked at in the disassembly whenever the compiler changes: 19 instructions
// between the test for EK_SLOT and the push.
template <>
__device__ __forceinline__ void slot_get6<float, 8>(const SlotFile<float, 8> &sf, int slot, float *t6) {
  typedef float V16 __attribute__((ext_vector_type(16)));
  const int s = __builtin_amdgcn_readfirstlane(slot);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const V16 w = __builtin_shufflevector(sf.f[2 * j], sf.f[2 * j + 1], 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
    t6[2 * j] = w[s];
    t6[2 * j + 1] = w[s + 8];
  }
}

// Four wide: the same trick needs sixteen-wide tuples of four vectors each, which cost 17 - 18 more registers and one
// wave per SIMD of k_filter_endpoints_pw (random_model(1005): 123 -> 141 VGPRs).  Here a tree of scalar branches over
// the slot, whose leaves read literal elements, serves: 2 compares and branches and six moves in place of 4 s_cmp +
// 4 s_cselect + 18 v_cndmask, with the registers and the occupancy of the plain build.  The barrier on each value
// keeps the leaves separate blocks (without it the compiler folds the tree back into the select chain).
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

template <>
__device__ __forceinline__ void slot_get6<float, 4>(const SlotFile<float, 4> &sf, int slot, float *t6) {
  slot_tree6<0, 4>(sf, __builtin_amdgcn_readfirstlane(slot), t6);
}

// No specialisation for the sixteen-wide file: the compiler's indexed moves are there already, and the tree measured
// worse (random_model(1002), k_edges_fused: 273 -> 290 spilled VGPRs, 53.7 -> 55.3 KB of code).  Float64 files and the
// literal slots of moving-box libraries (SpecSlots) are untouched as well.

}  // namespace mjpl
