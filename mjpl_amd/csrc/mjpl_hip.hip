// mjpl_hip.hip -- libmjpl_hip.so: gfx950 kernels + the C ABI of include/mjpl_hip.h.
//
// Replaces, for whole batches, the per-configuration body of the reference's
// CollisionConstraint.valid_config (src/mjpl/constraint/collision_constraint.py:26-30) and the
// edge discretisation of _valid_collision_interval (src/mjpl/planning/utils.py:188-216).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see __graft_entry__.py).
// There is deliberately no CPU fallback in this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <dlfcn.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mjpl_hip.h"
#include "mjpl_device.h"
#include "mjpl_filter.h"
#include "mjpl_pose.h"
#include "mjpl_project.h"
#include "mjpl_nearest.h"
#include "mjpl_nearest_cells.h"
#include "mjpl_contacts.h"
#include "mjpl_distance.h"
#include "mjpl_distance_grad.h"
#include "mjpl_push.h"
#include "mjpl_sweep.h"
#include "mjpl_topp.h"
#include "mjpl_jerk.h"
#include "mjpl_shortcut.h"
#include "mjpl_plan.h"
#include "mjpl_cplan.h"
#include "mjpl_roadmap.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

using namespace mjpl;

constexpr int kCtr = kCounterStride;  // ints between device counters: one 128-byte line each
constexpr int kNumCtr = kNumCounters;
constexpr size_t kFusedDbgWaves = 256 * 4 * 3 * 2;  // (wave slots of the chip, with room)
// workspace of one chunk of paths of mjpl_topp_profile* (one path may exceed it): the default of the option "topp_chunk_bytes"
constexpr size_t kToppChunkBytes = (size_t)512 << 20;
// workspace of one chunk of paths of mjpl_shortcut_paths* (one path may exceed it): the default of the option "shortcut_chunk_bytes"
constexpr size_t kShortcutChunkBytes = (size_t)256 << 20;
// workspace of one chunk of problems of mjpl_plan_paths* (one problem may exceed it): the default of the option "plan_chunk_bytes"
constexpr size_t kPlanChunkBytes = (size_t)256 << 20;
// the edge batch of one launch of mjpl_roadmap_build*, and the distance workspace of one search launch of mjpl_roadmap_query*
// whose graph does not fit in LDS: the default of the option "roadmap_chunk_bytes"
constexpr size_t kRoadmapChunkBytes = (size_t)256 << 20;
// the largest N whose distances mjpl_roadmap_query* keeps in LDS (144 KiB of the CU's 160): the default of "roadmap_lds_nodes"
constexpr int kRoadmapLdsNodes = 18432;

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return fail(MJPL_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                  __FILE__, __LINE__);                                                  \
  } while (0)

#define MJPL_TRY(...)                   \
  do {                                  \
    int _rc = (__VA_ARGS__);            \
    if (_rc != MJPL_OK) return _rc;     \
  } while (0)

// A device allocation that only grows.  reserve(n) frees, empties, then allocates, in that order: a failed hipMalloc
// leaves the buffer empty and the next launch tries again.  hipFree synchronises the device, so it is called only
// when a buffer must grow: steady-state launches call none.  The engine's buffers go with it (mjpl_destroy).
template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int release() {
    if (p) HIP_TRY(hipFree(p));
    p = nullptr;
    cap = 0;
    return MJPL_OK;
  }
  int reserve(size_t n, size_t at_least = 0) {  // (at_least: the smallest allocation worth making)
    if (n <= cap) return MJPL_OK;
    MJPL_TRY(release());
    n = std::max(n, at_least);
    HIP_TRY(hipMalloc(&p, n * sizeof(T)));
    cap = n;
    return MJPL_OK;
  }
};

// An arena's spans, listed once: run without a base the listing gives the byte count, with it the pointers.
struct Carver {
  char *base;
  size_t at = 0;
  template <class T>
  T *take(size_t count, size_t align = 256) {  // (the span's bytes rounded up to `align`)
    T *span = base ? (T *)(base + at) : nullptr;
    at += (count * sizeof(T) + align - 1) / align * align;
    return span;
  }
};

// What a nearest-neighbour look-up keeps between calls: its scratch, and what the last look-up ON THIS SCRATCH did.  The
// engine has one; the planner a second for the look-ups on its second stream (mjpl_rrt.h), which go with the planner.
struct NnScratch {
  DevBuf<char> parts;    // per-chunk partial results and the seed row
  DevBuf<char> arena;    // the screens' operands (binary16 rows), partial results, the cell-ordered scan's lists and sorted rows
  DevBuf<double> spare;  // distances of a ranged look-up whose caller wants none
  // (reset at the top of every look-up.  An offset into the arena, not a pointer: a reader that finds the arena smaller
  //  than the offset -- released, or never grown -- answers "unknown")
  struct Last {
    int path = 0;         // 0 float64 scan, 1 binary32 screen, 2 matrix-core screen (or 1: see its flag, mjpl_nearest_last_screen)
    bool cells = false;   // ... as the cell-ordered scan
    size_t count_at = 0;  // its candidate counts: byte offset in the arena, `waves` of them, of `nsub` sub-chunks
    int waves = 0, nsub = 0;
  } last;
};

// ------------------------------------------------------------------------------- kernels

// ---- exact path (float64): final verdicts --------------------------------------------------

template <int MAXS, bool WBOX, bool MBOX>
__global__ void __launch_bounds__(kBlock)
k_check_configs(const int *__restrict__ gip, int nip, const double *__restrict__ gdp, int ndp,
                const double *__restrict__ Q, int64_t N, int layout, uint8_t *__restrict__ valid,
                unsigned long long *__restrict__ bits, const int *__restrict__ ulist,
                const int *__restrict__ ucount, UndecidedConfigs uc, int32_t *__restrict__ first_bad) {
  extern __shared__ double smem[];
  const int B = blockDim.x;
  if (ulist && (int64_t)blockIdx.x * B >= (int64_t)*ucount) return;  // nothing left to re-run
  const int nplan = gip[H_NPLAN];
  Carve<double> c = carve_lds<double>(smem, gip, nip, gdp, ndp, nplan, 1, B);
  FkOut none = {};
  if (uc.count) {
    // patch mode: the rows of uc.q are undecided waypoints of edges; their number is read on the
    // device and may exceed what the grid covers in one pass: blocks stride over it
    const int64_t n = *uc.count < uc.cap ? *uc.count : uc.cap;
    for (int64_t base = (int64_t)blockIdx.x * B; base < n; base += (int64_t)gridDim.x * B) {
      const int64_t i = base + threadIdx.x;
      const bool active = i < n && uc.ga[i] < 0;  // pair-level items belong to k_patch_pairs
      load_columns(c.col0 + threadIdx.x, B, Q, n, i < n ? i : 0, nplan, layout, active);
      const bool hit = run_config<double, MAXS, false, WBOX, MBOX>(c.ip, c.tp, c.col0 + threadIdx.x, B,
                                                                   c.save + threadIdx.x, B, active, 0.0, none,
                                                                   i) == V_CONTACT;
      if (active && hit) {
        const int ed = uc.edge[i];
        valid[ed] = 0;
        // first_bad holds -1 (= UINT_MAX) for "valid so far": an unsigned min keeps the lowest index
        if (first_bad) atomicMin(reinterpret_cast<unsigned *>(first_bad) + ed, (unsigned)uc.idx[i]);
      }
    }
    return;
  }
  int64_t i;
  const bool active = pick_item(N, ulist, ucount, &i);
  load_columns(c.col0 + threadIdx.x, B, Q, N, i, nplan, layout, active);
  __syncthreads();
  const bool hit = run_config<double, MAXS, false, WBOX, MBOX>(c.ip, c.tp, c.col0 + threadIdx.x, B,
                                                               c.save + threadIdx.x, B, active, 0.0, none,
                                                               i) == V_CONTACT;
  if (valid && active) valid[i] = hit ? 0 : 1;
  if (bits) {
    unsigned long long m = __ballot(active && !hit);
    if ((threadIdx.x & 63) == 0 && active) bits[i >> 6] = m;
  }
}

__global__ void __launch_bounds__(kBlock)
k_fk(const int *__restrict__ gip, int nip, const double *__restrict__ gdp, int ndp,
     const double *__restrict__ Q, int64_t N, int layout, FkOut out) {
  extern __shared__ double smem[];
  const int B = blockDim.x;
  const int nplan = gip[H_NPLAN];
  Carve<double> c = carve_lds<double>(smem, gip, nip, gdp, ndp, nplan, 1, B);
  const int64_t i = (int64_t)blockIdx.x * B + threadIdx.x;
  const bool active = i < N;
  load_columns(c.col0 + threadIdx.x, B, Q, N, i, nplan, layout, active);
  __syncthreads();
  run_config<double, 1, true, true, true>(c.ip, c.tp, c.col0 + threadIdx.x, B, c.save + threadIdx.x, B,
                                          active, 0.0, out, i);
}

template <int MAXS, bool WBOX, bool MBOX>
__global__ void __launch_bounds__(kBlock)
k_check_edges(const int *__restrict__ gip, int nip, const double *__restrict__ gdp, int ndp,
              const double *__restrict__ QA, const double *__restrict__ QB, int64_t E, double step,
              int layout, int flags, uint8_t *__restrict__ valid, int32_t *__restrict__ first_bad,
              int *__restrict__ status, const int *__restrict__ rlist, const int *__restrict__ rcount) {
  UndecidedConfigs none = {};
  edge_body<double, MAXS, WBOX, MBOX>(gip, nip, gdp, ndp, QA, QB, E, step, layout, flags, 0.0, valid,
                                      first_bad, status, nullptr, nullptr, rlist, rcount, none);
}

// ---- filter path (float32): decides what it can, lists the rest ----------------------------

template <int MAXS, bool WBOX, bool MBOX>
__global__ void __launch_bounds__(kBlock)
k_filter_edges(const int *__restrict__ gip, int nip, const float *__restrict__ gfp, int nfp,
               const double *__restrict__ QA, const double *__restrict__ QB, int64_t E, double step,
               int layout, int flags, float tol, uint8_t *__restrict__ valid,
               int32_t *__restrict__ first_bad, int *__restrict__ status, int *__restrict__ ulist,
               int *__restrict__ ucount, UndecidedConfigs uc, const int *__restrict__ rlist,
               const int *__restrict__ rcount, int *__restrict__ zero_next) {
  zero_counters(zero_next);  // (only when this is the first kernel of the launch: one-pass mode)
  edge_body<float, MAXS, WBOX, MBOX>(gip, nip, gfp, nfp, QA, QB, E, step, layout, flags, tol, valid,
                                     first_bad, status, ulist, ucount, rlist, rcount, uc);
}

// (pose_project_lane, k_pose_apply, k_rrt_gen_project: mjpl_project.h -- per-model libraries instantiate them, too)

__global__ void __launch_bounds__(kPoseBlock)
k_pose_valid(const int *__restrict__ pi, const double *__restrict__ pd, const double *__restrict__ Q,
             int64_t N, uint8_t *__restrict__ valid, double *__restrict__ xpos, double *__restrict__ xmat) {
  extern __shared__ double smem[];
  constexpr int B = kPoseBlock;
  const int lane = threadIdx.x;
  const int nq = pi[PH_NQ];
  const double *tail = pd + pi[PH_OFF_TAIL];
  const double *jrange = pd + pi[PH_OFF_JRANGE];
  double *qw = smem + lane;
  const int64_t i = (int64_t)blockIdx.x * B + lane;
  const bool active = i < N;
  bool inside = true;
  for (int k = 0; k < nq; k++) {
    const double v = active ? Q[i * nq + k] : 0.0;
    qw[k * B] = v;
    inside = inside && (v >= jrange[2 * k] && v <= jrange[2 * k + 1]);
  }
  PoseChainOut o;
  pose_chain(pi, pd, qw, B, nullptr, 0, o);
  double dx[6], qs[4];
  pose_displacement(tail, o, dx, qs);
  if (active) {
    if (valid) valid[i] = (inside && norm6(dx) <= tail[PT_TOL]) ? 1 : 0;
    if (xpos) for (int k = 0; k < 3; k++) xpos[i * 3 + k] = o.site_xpos[k];
    if (xmat) for (int k = 0; k < 9; k++) xmat[i * 9 + k] = o.site_xmat[k];
  }
}


// (k_ik_solve: mjpl_project.h -- interpreting, or around a model's generated chain)

// ------------------------------------------------------------------------------- host model

struct HostModel {
  int nq = 0, njnt = 0, nbody = 0, ngeom = 0;
  std::vector<int> body_parentid, body_weldid, body_jntadr, body_jntnum;
  std::vector<double> body_pos, body_quat;
  std::vector<int> jnt_type, jnt_qposadr;
  std::vector<double> jnt_axis, jnt_pos, qpos0;
  std::vector<int> geom_type, geom_bodyid, geom_contype, geom_conaffinity;
  std::vector<double> geom_size, geom_pos, geom_quat, geom_rbound, geom_margin;
};

// What the compiler derives once from the model, the allowed body pairs and the planning selection, and every later
// stage and table builder reads (mjpl_compile.h: layout_model).
struct ModelLayout {
  // world-welded bodies and geoms, their folded poses (FK output reads them)
  std::vector<char> body_static, geom_static;
  std::vector<double> st_xpos, st_xquat, st_xmat, st_gxpos, st_gxmat;
  std::vector<int> world_row;  // static geom -> its row of the world tables (-1: a moving geom)
  std::vector<int> winfo;      // world row -> geom type | geom id << 8
  // moving bodies in id order; parent_src[k] of order[k]: PARENT_STATIC, PARENT_CUR or LDS save slot + 1; save_slot per body
  std::vector<int> order, parent_src, save_slot;
  // moving geoms in processing order (stage_of: geom -> index in mgeoms, -1: static); per stage the last stage that
  // reads it, its register slots, its static partners (geom ids) and stored ones (earlier stages)
  std::vector<int> mgeoms, stage_of, last_user, slot_of;
  std::vector<std::vector<int>> world_partners, stored_partners;
  std::vector<int> col_of;  // qpos address -> planning column (-1: constant)
  int nslots = 0, nsave = 0, maxs = 4;
  bool wbox = false, mbox = false;
  int npairs = 0, npairs_world = 0, nmoving = 0, nplanes = 0;  // (nmoving: moving geoms; nplanes: static planes)
  int npruned = 0;  // enabled pairs (counted in npairs) on no partner list: proved never to pass their cull
  int nworld() const { return (int)winfo.size(); }  // static geoms: every one has a row
  int moving_base() const { return mgeoms.empty() ? 0 : mgeoms[0]; }  // model id of the first moving geom
};

// The filter's binary32 error bound and what follows from it (mjpl_compile.h: filter_error_bound)
struct FilterBound {
  double ferr_a = 0, ferr_b = 0;  // |pose error| <= ferr_a + ferr_b * max coordinate
  double fmax_coord = 0;
  float tol = 1e-4f;              // tolerance band in force (>= what was asked for)
  bool usable = true;             // false: this model's binary32 error floor is too high, exact path only
  int npoisoned = 0;              // static geoms too large / far for binary32: their pairs are always undecided
  std::vector<int> poison_rows;   // ... their world rows: NaN in the float image
};

template <class T>
std::vector<T> copy_n(const T *p, size_t n) {
  return std::vector<T>(p, p + n);
}

// entry points of a per-model specialised library (see load_spec)
struct SpecLib {
  typedef int (*ConfigsFn)(hipStream_t, unsigned, unsigned, size_t, const int *, int, const float *, int, const double *,
                           int64_t, int, float, uint8_t *, int *, int *, UndecidedConfigs, int *);
  typedef int (*EndpointsFn)(hipStream_t, unsigned, unsigned, size_t, const int *, int, const float *, int, const double *,
                             const double *, int64_t, int, float, uint8_t *, int32_t *, int *, int *, int *, UndecidedConfigs,
                             int *, int *, ItemBuffers, double, int *);
  typedef int (*PatchFn)(hipStream_t, unsigned, unsigned, size_t, const int *, int, const double *, int, GeomTable,
                         UndecidedConfigs, uint8_t *, int32_t *);
  typedef int (*ItemsFn)(hipStream_t, unsigned, unsigned, size_t, const int *, int, const float *, int, ItemBuffers, EdgeSource, float,
                         uint8_t *, int32_t *, int *, int *, UndecidedConfigs);
  typedef int (*EndpointsPwFn)(hipStream_t, size_t, const int *, int, const float *, int, const double *, const double *, int64_t, int,
                               float, uint8_t *, int32_t *, int *, int *, int *, UndecidedConfigs, ItemBuffers, double, int *, int *);
  typedef int (*ItemsPwFn)(hipStream_t, size_t, const int *, int, const float *, int, ItemBuffers, EdgeSource, float, uint8_t *,
                           int32_t *, int *, int *, UndecidedConfigs, int *);
  typedef int (*TailFn)(hipStream_t, size_t, TailArgs);
  typedef int (*FusedFn)(hipStream_t, int, size_t, FusedArgs);  // (waves per workgroup, LDS bytes, arguments)
  FusedFn fused = nullptr;
  FusedFn fused_f64 = nullptr;  // the float64 pool kernel around the model's generated check (mjpl_spec_launch_fused_f64), if it has one
  int fused_waves = kFusedWaves;  // what its fused kernel was built for (mjpl_spec_fused_waves)
  bool fused_cert = false;        // ... and whether with the edge certificate (mjpl_spec_fused_cert): LDS rows of |QB - QA|
  // generated PoseConstraint projections, one per site body of the model (mjpl_project.h): chain hashes and launchers
  // (row kernels of mjpl_rows.h: projection index, lanes per row, stream, waves, ...; 0 launched, -1 refused, -2 HIP error)
  typedef int (*PoseApplyFn)(int, int, hipStream_t, unsigned, const int *, const double *, const double *, const double *, int64_t, int64_t,
                             double *, uint8_t *, int32_t *, PosePhase);
  typedef int (*GenProjectFn)(int, int, hipStream_t, unsigned, int, int, int, double, int, const int *, const double *, const int *,
                              const double *, const uint8_t *, const double *, const double *, const double *, RrtLanes, RrtCand, int *);
  typedef int (*IkSolveFn)(int, int, hipStream_t, unsigned, const int *, const double *, const double *, int64_t, int64_t, double *, uint8_t *,
                           int32_t *, double *, int, unsigned long long);
  int pose_count = 0;
  unsigned long long (*pose_hash)(int) = nullptr;
  PoseApplyFn pose_apply = nullptr;
  GenProjectFn gen_project = nullptr;
  IkSolveFn ik_solve = nullptr;
  EndpointsPwFn endpoints_pw = nullptr;
  ItemsPwFn items_pw = nullptr;
  TailFn tail = nullptr;
  void *lib = nullptr;
  int generic_rows = 0, generic_stages = 0;  // scene-generic libraries: rows per moving geom, moving geoms
  ConfigsFn configs = nullptr;
  EndpointsFn endpoints = nullptr;
  ItemsFn items = nullptr;
  PatchFn patch = nullptr;
};

// The planner's knobs (options "rrt_<field>"; mjpl_rrt_create copies the engine's into the handle it makes).
struct RrtTuning {
  // The connect phase's nearest neighbours, early (round 5).  A lane's round does not depend on any other lane's (both trees
  // are the round's snapshot), and the tail of the first extension is a handful of lanes taking a thousand sequential steps
  // on an otherwise idle chip: once no more than `early_lanes` lanes are still extending, the lanes that are through get
  // their nearest node of the OTHER tree on a second stream (what they reached is final: ln.C of a lane with act == 0);
  // the second extension then looks up only the lanes that were still under way, and waits for the early answers.  The
  // same queries against the same nodes: the same nodes.  `early_min_nodes`: from what size of the other tree on (tests
  // set both thresholds low); `early_next`: the next round's look-up as well.
  // (With the chains capped the last chunks are a millisecond and the look-ups two or three: rounds of 13.0 - 13.5 ms with
  //  it at any threshold, 13.1 without (profiles/r06_rrt_early_ab.txt, one box): OFF by default from round 6 on -- one
  //  stream, one scratch arena --, still an option and still tested.)
  int early_nn = 0, early_lanes = 4096, early_next = 1;
  int64_t early_min_nodes = 65536;
  // projecting extensions: most steps a lane takes per chunk, and the candidate slots a chunk is sized for
  // (round 4, with the chain as generated code a step is cheap enough for the chunk's fixed cost to show: 64 / 65 536 ->
  //  65.2 ms per 131 072-lane round, 256 / 262 144 -> 62.6, 1 024 / 1 048 576 -> 59.8; the slots are bounded by the
  //  candidate buffer, 4 L, all the same)
  int proj_steps = 1024;
  int64_t proj_slots = 1 << 20;
  // ... and the shape of the generating launch (mjpl_rows.h; rows_shape), both there for A/B timing: lanes per row (0: by
  // the number of active lanes; 1 / 4 / 8 / 16 / 64 forced), waves per launch (one per SIMD: the kernels' registers)
  int proj_g = 0, proj_waves = 1024;
  // rows of sixteen lanes that run a step ahead (mjpl_rows.h: k_rrt_gen_project_ahead), when no more than `ahead_lanes`
  // lanes extend: one row per wave (measured: with four rows per wave, 1 536 lanes, 14.0 ms against 13.5 with eight lanes
  // per row -- the statements of running ahead are paid by every row of the wave; one row per wave, 268 lanes x 1 024
  // steps: 20.5 ms against 23.9).  ahead = 0: never
  int ahead = 1, ahead_lanes = 1024;
};

}  // namespace

struct mjpl_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop{};
  HostModel m;
  std::set<std::pair<int, int>> allowed;  // sorted body-id pairs (collision_constraint.py:60-64)
  std::vector<int> qidx;
  std::vector<double> qbase;
  // compiled program
  std::vector<int> ip;
  std::vector<double> dp;
  std::vector<float> fp;  // the filter's float32 image of dp (cull bounds widened by filter_tol)
  int *d_ip = nullptr;
  double *d_dp = nullptr;
  float *d_fp = nullptr;
  int *d_status = nullptr;
  // float32 filter + exact re-run of what it cannot decide
  bool filter = true;
  float filter_tol_req = 1e-4f;   // what the caller (or the default) asked for
  bool filter_tol_user = false;   // asked for through mjpl_set_filter / MJPL_FILTER_TOL
  FilterBound fb;                 // the band in force, and whether the filter serves this model at all
  // option "prune_pairs": the program leaves out the enabled pairs proved never to pass their bounding cull (mjpl_compile.h:
  // prune_pairs) -- 1: pairs of a moving geom with a static geom or a plane, 2: pairs of two moving geoms of one chain as well;
  // `pruned` holds them as (g1 < g2), found once per model, level and tolerance asked for
  int prune_pairs = 1, pruned_level = 0;
  std::set<std::pair<int, int>> pruned;
  bool pruned_valid = false, pruned_tol_user = false;
  float pruned_tol_req = 0.0f;
  int prune_evals = 0;  // cell evaluations the proofs took (of kPruneModelEvals); read-only option "prune_evals"
  // option "prune_contacts": pairs of a moving geom with a static geom or a plane proved never to come within their margin
  // (mjpl_compile.h: prune_contacts) -- a side set of the program: in no table, mixed into program_hash when non-empty, left
  // out by a per-program library's generated check only.  1: on, >= 2: on with that many cell evaluations per pair (tests)
  int prune_contacts = 1, never_level = 0;
  std::set<std::pair<int, int>> never_touch, never_from;  // (never_from: the dropped pairs the set was found beside)
  bool never_valid = false;
  double never_tol = 0, never_poison_slack = 0;
  std::vector<int> never_poison_rows;
  int prune_contact_evals = 0;  // cell evaluations (of kContactModelEvals); read-only option "prune_contact_evals"
  uint64_t program_hash = 0;      // FNV-1a of the compiled tables (ip, fp, dp), the kernel variant, the header digest and the never-touch set when it is not empty
  const SpecLib *spec = nullptr;  // this model's own filter kernels, if a library for program_hash was found
  // ... or, failing that, a scene-generic library of the ROBOT (robot_hash: moving bodies, their geoms and
  // self pairs, planning set, tolerance -- nothing of the static geoms): its generated code takes every
  // static partner's cull row from a table in front of the float32 tables (scene_floats of them), so the
  // obstacles may change without a compiler
  bool spec_generic = false;
  uint64_t robot_hash = 0;
  std::vector<float> scene;      // [scene header | per moving geom: kSceneRows rows of 8] (compile_program)
  float *d_fp_base = nullptr;    // allocation behind d_fp (= d_fp_base + scene.size())
  bool spec_off = false;          // mjpl_set_spec(e, 0): run the interpreting kernels whatever libraries exist
  bool spec_generic_only = false; // mjpl_set_spec(e, 2): pass over the program's own library, take the robot's scene-generic one
  DevBuf<int> d_ulist;      // items (configurations / whole edges) the filter left undecided
  int *d_ucount_base = nullptr;  // both counter sets; d_ucount = the one the last launch used
  bool counters_stale = false;
  int *d_ucount = nullptr;  // [0] how many of those, [1] undecided waypoints of edges, [2] edges in d_slist
  DevBuf<int> d_slist;      // two-pass edge filter: edges whose endpoint passed
  bool two_pass = true;
  // timing runs (mjpl_time_edges_stages_dev): marks[k] is recorded after stage k - 1 of the launch
  // (marks[0] at its start); nullptr in ordinary launches
  hipEvent_t *marks = nullptr;
  // option "kernel_timer" (bench.py: every line's roofline from THIS run), a bit mask: 1 = the dominant kernel of the configuration /
  // projection / IK / planner-extension launches is bracketed with events, 2 = the nearest-neighbour scans; "kernel_timer_ms" /
  // "kernel_timer2_ms" read the sums since the option was set, "kernel_timer[2]_launches" how many
  int kt_mode = 0, kt_used[2] = {0, 0};  // (kt_mode: bit 0 = class 1, bit 1 = class 2)
  std::vector<hipEvent_t> kt_ev[2];
  // undecided waypoints, uc_cap of each (uc_reserve): rows of nplan float64 (allocated as rows of nq), edge, check index, geom pair
  DevBuf<double> d_ucq;
  DevBuf<int> d_ucedge, d_ucidx, d_ucga, d_ucgb;
  double *d_geomtab = nullptr;  // GTB_LEN doubles per model geom (k_patch_pairs)
  // lane-per-waypoint interior pass: (edge, idx) items, long-edge list
  DevBuf<double> d_tstep, d_itemck;  // (checkpoint rows: allocated by the first launch with long items)
  DevBuf<int> d_itemedge, d_itemidx, d_llist;
  int *d_icount = nullptr;
  DevBuf<int> d_eclaim;  // [llist_cap] per-edge claim word: the launch generation that listed the edge in d_ulist
  int claim_gen = 0;
  size_t item_cap = 0, llist_cap = 0;
  bool expand = true;
  // endpoint and item kernels as persistent grids of waves with tile queues (queued interpreter only).
  // -1: where it pays -- a model's own specialised kernels (0.257 -> 0.245 ms per step); the interpreting
  // kernels, whose waves differ more in what a tile costs them, are faster as ordinary grids (0.397 vs
  // 0.459 ms).  MJPL_PERSIST=0 / 1 forces either (tests run both ways).
  int persist = -1;
  bool fused_tail = true;  // MJPL_TAIL: walking kernel, pair re-check and exact edge kernel as roles of one launch (k_tail)
  // ONE filter kernel per edge launch (k_edges_fused, mjpl_fused.h): endpoint and waypoint tiles served by the same
  // resident workgroups from a work pool in LDS.  MJPL_FUSED=0 restores the two persistent kernels;
  // MJPL_FUSED_POLICY (bit 0: item tiles first), MJPL_FUSED_KMAX: A/B measurements
  bool fused = true;
  int fused_policy = 0, fused_kmax = 4096, fused_pool_cap = 0;  // (MJPL_FUSED_POOL: at most that many ring slots)
  bool f64_spec = true;  // the float64 pool kernel around the library's generated check, when it has one (MJPL_F64_SPEC=0: interpreting)
  const SpecLib *spec_cert = nullptr;  // the model's library built WITH the edge certificate (spec/cert/), if there is one ...
  int64_t fused_cert_min_edges = (int64_t)1 << 20;  // ... takes the fused launches of at least this many edges (option "fused_cert_min_edges"; 0: never)
  int fused_cert = 1;  // the fused kernel's edge certificate (mjpl_fused.h; MJPL_FUSED_CERT=0: every surviving edge's waypoints are checked)
  bool fused_mbox = false;
  bool f64_queued = true;  // MJPL_F64_QUEUED: the float64 pool kernel checks through the candidate queues (A/B switch)
  int fused_single_max = 32768;  // MJPL_FUSED_SINGLE: batches up to this many edges check every configuration of an edge in one round (measured: 0.068 vs 0.087 ms at 1 024 edges, 0.090 vs 0.102 at 32 768, 0.116 vs 0.106 at 65 536)
  const char *fused_dbg_path = nullptr;  // MJPL_FUSED_DEBUG=<file> (with a -DMJPL_FUSED_DEBUG build of the kernels)
  DevBuf<unsigned long long> d_fused_dbg;
  size_t item_cap_limit = (size_t)1 << 26;  // MJPL_ITEM_CAP: edges beyond it take the walking kernel
  NnScratch nn;                 // nearest neighbour: the scratch of the look-ups on the engine's stream
  int nn_mfma = 1;              // MJPL_NN_MFMA=0: binary32 screen only
  int64_t nn_reserve_nodes = 0; // packed-node rows the screened look-up's scratch is sized for at least (mjpl_rrt_create: the planner's capacity, 2^23 at most)
  int64_t nn_sample = 65536;    // MJPL_NN_SAMPLE: nodes of the strided sample the matrix cores take every query's bound from
  // switches that used to be read from the environment wherever they were used (round 6: options, include/mjpl_hip.h)
  size_t zero_copy_bytes = (size_t)256 << 10;  // "zero_copy_bytes"
  int rows_g = 0;               // "rows_g": lanes per row of the projection / IK row kernels forced (0: by the batch size)
  int pose_spec = 1;            // "pose_spec": 0 = projections and IK seeds on the interpreting kernels
  int pose_phase_steps = 0;     // "pose_phase_steps"
  int rrt_trace = 0;            // "rrt_trace": 1 = a planner round's phases on stderr, 2 = every extension chunk (synchronises)
  RrtTuning rrt;                // "rrt_early_nn" ... "rrt_proj_waves"
  int nn_cells = 1;             // the cell-ordered scan for big trees (mjpl_nearest_cells.h); option "nn_cells"
  int64_t nn_cells_min = 131072; // ... from this many nodes on; option "nn_cells_min_nodes"
  int64_t nn_cells_sample = 32768; // ... with bounds from a strided sample of this many nodes ("nn_cells_sample"; measured on the planner's trees,
                                 //     ms per look-up targets / connect phase: 8 192: 4.79 / 2.83, 16 384: 4.55 / 2.61, 32 768: 4.64 / 2.68, 65 536: 5.02 / 2.83)
  // options, both OFF: every query's bound tightened on its home sub-chunks before the candidate pass; a binary32 second screen
  // of the parked pairs.  Measured on one box, 14 planner rounds (profiles/README.md round 6): the second screen 21.2 ms per
  // round against 19.5 without (it evaluates every parked pair twice where the first evaluation decides most), the home pass
  // 19.6 (what it saves the scan it costs itself).  Kept for trees and batches of other shapes.
  int nn_home = 0, nn_second_screen = 0;
  int nn_probe = 0;             // option "nn_probe" (2: count the exact evaluations)
  size_t uc_cap = 0, uc_cap_limit = 0;
  ModelLayout lay;  // static poses for FK output, slot and save counts, kernel shape
  // the immediate (non-queued) interpreter serves models with moving boxes and models that keep
  // more than 16 geoms in the slot file (one general <32, true, true> build)
  // Which builds a model runs.  Exact kernels: <4|8|16, wbox, false>, or the general <32, true, true>
  // for moving boxes / more than 16 stored geoms.  Filter kernels: the same small builds, then
  // <24, true, true> -- still the queued interpreter, moving boxes through its box queue -- and
  // only beyond 24 stored geoms the immediate interpreter <32, true, true>.
  bool exact_general() const { return lay.mbox || lay.maxs > 16; }
  bool force_immediate = false;  // MJPL_FORCE_IMMEDIATE (create-time, tests)
  bool immediate() const { return lay.nslots > kQueuedMaxSlots || (force_immediate && exact_general()); }
  bool filter_mbox() const { return exact_general() && !immediate(); }
  // RCCL communicator of the frontier planner's exchange (mjpl_comm_init); none = a world of one
  void *comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  // grow-only device staging slots: a host-pointer entry point's inputs and outputs (staged()), the program of an IK
  // solve, the parked-row list of a two-launch projection
  DevBuf<char> stage_in, stage_out, stage_ik, stage_parked;
  // pinned, grow-only host block of the small-batch tiers of staged()
  void *h_pin = nullptr;
  size_t h_pin_bytes = 0;
  // candidate pairs of mj_collision for mjpl_contacts* (build_contact_table): made once at create from the model
  // alone, so mjpl_set_planning leaves them be.  Rows as the caller sees them (smaller geom type first) and the
  // kernel's records (mjpl_contacts.h: CI_* / CD_*)
  std::vector<int32_t> ct_g1, ct_g2;
  std::vector<uint8_t> ct_allowed;
  int ct_unsupported = -1;  // index of a candidate pair no narrowphase routine here decides (-1: none)
  int *d_ct_ip = nullptr;
  double *d_ct_dp = nullptr;
  DevBuf<double> d_ct_scratch;  // FK scratch rows of one launch
  // distance table of mjpl_distances* / mjpl_clearance* (mjpl_distance.h: DT_*), made at mjpl_create from the model
  double *d_dt = nullptr;
  // column / joint / geom tables of mjpl_clearance_grad* (mjpl_distance_grad.h: GC_*, JR_*), made at mjpl_create and
  // remade by mjpl_set_planning; body pose scratch rows of one launch (grow-only)
  double *d_gr = nullptr;
  DevBuf<double> d_gr_scratch;
  // column frames scratch rows of one mjpl_near_pairs* launch (mjpl_distance.h: NearOut::frames; grow-only)
  DevBuf<double> d_nr_frames;
  // mjpl_push_out* (mjpl_push.h): the largest margin of a non-allowed candidate pair (0 without one), made with the
  // candidate table; per chunk the two work buffers of rows with their ids and fill counters, and the near-pair outputs
  // of the active rows (grow-only); the pinned word the host reads a counter into
  double ct_margin_max = 0.0;
  DevBuf<double> d_push_f64;
  DevBuf<int> d_push_i32;
  int *h_push_n = nullptr;
  // mjpl_sweep_* (mjpl_sweep.h): the bounds in force over the planning columns (empty: none) and the device table
  // [lo | hi | W] made from them (mjpl_compile.h: build_sweep_table; not part of the hashed program); per chunk the two
  // work buffers of nodes, the measurements of a round and the per-edge hit keys (grow-only)
  std::vector<double> sweep_lo, sweep_hi;
  double *d_sweep_tab = nullptr;
  DevBuf<double> d_sweep_rows[2], d_sweep_hd[2], d_sweep_f64;
  DevBuf<int> d_sweep_meta[2], d_sweep_i32;
  DevBuf<unsigned long long> d_sweep_key;
  // mjpl_sweep_splines*: the call's tables [wp_off | per piece: first row, n - 1] on the host (what the upload reads:
  // rewritten only after the stream has drained) and on the device; M for a caller that wants none (grow-only)
  std::vector<int64_t> sweep_piece_h;
  DevBuf<int64_t> d_sweep_piece;
  DevBuf<double> d_sweep_M;
  // mjpl_topp_* (mjpl_topp.h): the call's offset tables [wp_off | samp_off] and limits [vmin | vmax | amin | amax] on
  // the host (what the uploads read: rewritten only after the stream has drained) and on the device; c' of the Thomas
  // recurrence, grown to the longest path seen; the workspace of a chunk of paths (all grow-only)
  std::vector<int64_t> topp_off_h;
  std::vector<double> topp_lim_h, topp_cp_h;
  DevBuf<int64_t> d_topp_off;
  DevBuf<double> d_topp_lim, d_topp_cp, d_topp_ws;
  // option "topp_chunk_bytes": the workspace of one chunk of paths (tests: chunk boundaries at small shapes; the number of
  // launches changes, no bit of any output); read-only option "topp_last_chunks": chunks of the last mjpl_topp_profile*
  int64_t topp_chunk_bytes = (int64_t)kToppChunkBytes;
  int64_t topp_last_chunks = 0;
  // mjpl_shortcut_paths* (mjpl_shortcut.h): the call's offsets on the device, and per chunk of paths the live lists, arc
  // lengths, candidates, the round's edge batch with its verdicts and rocPRIM's scan space (one arena: carve_shortcut),
  // and the round's header.
  DevBuf<int64_t> d_sc_off;
  DevBuf<char> d_sc_arena;
  DevBuf<unsigned long long> d_sc_head;
  // option "shortcut_chunk_bytes": the workspace of one chunk of paths (more or fewer launches, no bit of any output);
  // read-only: "shortcut_last_chunks", and what the last call validated and -- with "kernel_timer" & 1 -- spent per phase
  int64_t shortcut_chunk_bytes = (int64_t)kShortcutChunkBytes;
  int64_t shortcut_last_chunks = 0, shortcut_last_rounds = 0, shortcut_last_edges = 0;
  double shortcut_last_ms[3] = {0, 0, 0};  // propose (with scan and gather), validate, commit
  // mjpl_plan_paths* (mjpl_plan.h): the sampling box, and per chunk of problems the trees with their parents, the
  // round's targets, the ends' batch, the round's edge batch with its verdicts and rocPRIM's scan space (one arena, which
  // the constrained calls share: carve_plan, carve_cplan), and the round's header.
  DevBuf<double> d_pl_box;
  DevBuf<char> d_pl_arena;
  DevBuf<unsigned long long> d_pl_head;
  DevBuf<int> d_pl_q;  // mjpl_plan_paths_constrained* (mjpl_cplan.h): the planning columns and their inverse
  // option "plan_chunk_bytes": the workspace of one chunk of problems (more or fewer launches, no bit of any output);
  // read-only: "plan_last_chunks", and what the last call validated and -- with "kernel_timer" & 1 -- spent per phase
  int64_t plan_chunk_bytes = (int64_t)kPlanChunkBytes;
  int64_t plan_last_chunks = 0, plan_last_rounds = 0, plan_last_edges = 0;
  double plan_last_ms[4] = {0, 0, 0, 0};  // propose (with scan and gather), validate, commit; constrained: project
  // mjpl_roadmap_build* / mjpl_roadmap_query* (mjpl_roadmap.h): the configuration batch, the neighbour lists and the edge
  // batch; the lists' indices, counts, flags and verdicts; the sort keys; rocPRIM's sort and scan space (one arena:
  // carve_roadmap_build, carve_roadmap_query); the call's header.  Nothing of a graph stays here between calls: the
  // caller's arrays hold it.
  DevBuf<char> d_rm_arena;
  DevBuf<unsigned long long> d_rm_head;
  // options "roadmap_chunk_bytes" and "roadmap_lds_nodes" (more or fewer launches, no bit of any output); read-only: what
  // the last call did and -- with "kernel_timer" & 1 -- spent per phase (build: nodes, neighbours, validate, graph;
  // query: attach, validate, search with the walk)
  int64_t roadmap_chunk_bytes = (int64_t)kRoadmapChunkBytes;
  int64_t roadmap_lds_nodes = kRoadmapLdsNodes;
  int64_t roadmap_last_edges = 0, roadmap_last_chunks = 0, roadmap_last_sweeps = 0;
  double roadmap_last_ms[4] = {0, 0, 0, 0};
};

namespace {

constexpr size_t kStageFloor = 1 << 16;  // a staging slot is never smaller (DevBuf::reserve: at_least)

// ---- per-model specialised filter kernels (mjpl_amd/specialise.py builds them) ----
// A library libmjpl_spec_<hash>.so holds the three float32 filter kernels of mjpl_filter.h instantiated
// with generated straight-line code for ONE compiled program.  It is looked up by the program's hash
// in $MJPL_SPEC_DIR (default: the directory `spec` next to this library); MJPL_SPEC=0 disables it.
// The cache belongs to the process, engines to their threads ("one engine per thread", include/mjpl_hip.h):
// every look-up and insertion happens under spec_mutex().  Entries are never erased and std::map never moves
// its nodes, so the pointer an engine keeps stays valid without the lock.
std::map<uint64_t, SpecLib> &spec_cache() {
  static std::map<uint64_t, SpecLib> c;
  return c;
}
std::mutex &spec_mutex() {
  static std::mutex m;
  return m;
}

// mjpl_set_spec_dir: per-model libraries are looked for there instead of beside this library (process-wide)
std::string &spec_dir_store() {
  static std::string d;
  return d;
}
std::string spec_dir_override() {
  std::lock_guard<std::mutex> lock(spec_mutex());
  return spec_dir_store();
}

// dlopen <dir>/<prefix><hash>.so and check that it was built for this hash from these headers
const SpecLib *find_spec(uint64_t hash, bool generic, const char *subdir = nullptr) {
  std::string dir_override = spec_dir_override();
  std::lock_guard<std::mutex> lock(spec_mutex());
  auto &cache = spec_cache();
  uint64_t key = hash ^ (generic ? 0x9e3779b97f4a7c15ull : 0ull);
  if (subdir) {  // (a build of another kind beside the default ones: spec/cert/ holds the edge-certificate builds)
    if (dir_override.empty()) {
      Dl_info info0;
      if (dladdr((const void *)&mjpl_version, &info0) && info0.dli_fname) {
        dir_override = info0.dli_fname;
        const size_t slash0 = dir_override.rfind('/');
        dir_override = (slash0 == std::string::npos ? std::string(".") : dir_override.substr(0, slash0)) + "/spec";
      }
    }
    dir_override += std::string("/") + subdir;
  }
  const char *env_dir = dir_override.empty() ? nullptr : dir_override.c_str();
  if (env_dir)  // (libraries of another directory are other libraries: e.g. the certificate builds under spec/cert)
    for (const char *c = env_dir; *c; c++) key = (key ^ (uint64_t)(unsigned char)*c) * 0x100000001b3ull;
  auto it = cache.find(key);
  if (it != cache.end()) return it->second.lib ? &it->second : nullptr;
  SpecLib sl;
  std::string dir;
  if (env_dir) {
    dir = env_dir;
  } else {
    Dl_info info;
    if (dladdr((const void *)&mjpl_version, &info) && info.dli_fname) {
      dir = info.dli_fname;
      const size_t slash = dir.rfind('/');
      dir = (slash == std::string::npos ? std::string(".") : dir.substr(0, slash)) + "/spec";
    }
  }
  char name[64];
  snprintf(name, sizeof(name), "/libmjpl_spec%s_%016llx.so", generic ? "g" : "", (unsigned long long)hash);
  void *lib = dir.empty() ? nullptr : dlopen((dir + name).c_str(), RTLD_NOW | RTLD_LOCAL);
  if (lib) {
    auto abi = (int (*)())dlsym(lib, "mjpl_spec_abi");
    auto hashf = (unsigned long long (*)())dlsym(lib, "mjpl_spec_hash");
    auto stamp = (unsigned long long (*)())dlsym(lib, "mjpl_spec_src_stamp");
    auto gen = (int (*)())dlsym(lib, "mjpl_spec_generic");  // 0, or rows per moving geom << 8 | moving geoms
    sl.configs = (SpecLib::ConfigsFn)dlsym(lib, "mjpl_spec_launch_configs");
    sl.endpoints = (SpecLib::EndpointsFn)dlsym(lib, "mjpl_spec_launch_endpoints");
    sl.items = (SpecLib::ItemsFn)dlsym(lib, "mjpl_spec_launch_items");
    sl.patch = (SpecLib::PatchFn)dlsym(lib, "mjpl_spec_launch_patch");
    sl.endpoints_pw = (SpecLib::EndpointsPwFn)dlsym(lib, "mjpl_spec_launch_endpoints_pw");
    sl.items_pw = (SpecLib::ItemsPwFn)dlsym(lib, "mjpl_spec_launch_items_pw");
    sl.tail = (SpecLib::TailFn)dlsym(lib, "mjpl_spec_launch_tail");
    sl.fused = (SpecLib::FusedFn)dlsym(lib, "mjpl_spec_launch_fused");
    sl.fused_f64 = (SpecLib::FusedFn)dlsym(lib, "mjpl_spec_launch_fused_f64");
    if (auto fw = (int (*)())dlsym(lib, "mjpl_spec_fused_waves")) sl.fused_waves = fw();
    if (auto fc = (int (*)())dlsym(lib, "mjpl_spec_fused_cert")) sl.fused_cert = fc() != 0;
    sl.pose_hash = (unsigned long long (*)(int))dlsym(lib, "mjpl_spec_pose_hash");
    sl.pose_apply = (SpecLib::PoseApplyFn)dlsym(lib, "mjpl_spec_launch_pose_apply");
    sl.gen_project = (SpecLib::GenProjectFn)dlsym(lib, "mjpl_spec_launch_gen_project");
    sl.ik_solve = (SpecLib::IkSolveFn)dlsym(lib, "mjpl_spec_launch_ik_solve");
    if (auto pc = (int (*)())dlsym(lib, "mjpl_spec_pose_count"))
      sl.pose_count = (sl.pose_hash && sl.pose_apply && sl.gen_project && sl.ik_solve) ? pc() : 0;
    // (the stamp: both libraries built from the same mjpl_filter.h / mjpl_device.h / mjpl_trig.h -- the
    // structs that cross this boundary by value and the table layouts live there)
    const int g = gen ? gen() : 0;
    if (abi && hashf && stamp && abi() == MJPL_SPEC_ABI && stamp() == (unsigned long long)MJPL_SRC_STAMP && hashf() == hash &&
        (g != 0) == generic && sl.configs && sl.endpoints && sl.items && sl.patch && sl.endpoints_pw && sl.items_pw && sl.tail && sl.fused) {
      sl.lib = lib;
      sl.generic_rows = g >> 8;
      sl.generic_stages = g & 255;
    } else {
      dlclose(lib);
    }
  }
  auto ins = cache.emplace(key, sl).first;
  return ins->second.lib ? &ins->second : nullptr;
}

// `generic_ok`: the program satisfies what a scene-generic library assumes (compile_program)
void load_spec(mjpl_engine *e, bool generic_ok = false, int nstage = 0) {
  e->spec = nullptr;
  e->spec_generic = false;
  e->spec_cert = nullptr;  // (before the early return: a certificate build never outlives the default library it was found beside)
  if (e->spec_off || e->immediate() || (e->exact_general() && !e->filter_mbox()) || !e->fb.usable) return;  // (the generator covers the queued builds)
  if (!e->spec_generic_only) e->spec = find_spec(e->program_hash, false);
  // (round 6: the certificate pays from about a million edges per launch on -- +7 ... 11 % -- and costs 4 % at 262 144,
  //  profiles/README.md round 5: both builds are loaded, launch_edges picks by the batch's size)
  if (e->spec && !e->spec->fused_cert) {
    const SpecLib *c = find_spec(e->program_hash, false, "cert");
    if (c && c->fused_cert && c->fused_waves == e->spec->fused_waves) e->spec_cert = c;
  }
  if (e->spec || !generic_ok) return;
  const SpecLib *g = find_spec(e->robot_hash, true);
  if (g && g->generic_rows == kSceneRows && g->generic_stages == nstage) {
    e->spec = g;
    e->spec_generic = true;
  }
}

}  // namespace

#include "mjpl_compile.h"

namespace {

// Replace a create-time device table by a host vector: the old block is freed first, and a failed allocation or copy
// leaves the slot null (an empty vector, too: nothing is allocated for it).
template <class T>
int upload_table(T **slot, const std::vector<T> &host) {
  T *old = *slot;
  *slot = nullptr;
  if (old) HIP_TRY(hipFree(old));
  if (host.empty()) return MJPL_OK;
  T *d = nullptr;
  HIP_TRY(hipMalloc(&d, host.size() * sizeof(T)));
  const hipError_t err = hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    (void)hipFree(d);
    HIP_TRY(err);
  }
  *slot = d;
  return MJPL_OK;
}

// Compile the model into the ip/dp program the kernels interpret (mjpl_compile.h: stages 1 to 6 on the host), find
// its library and put the tables on the device.
int compile_program(mjpl_engine *e) {
  MJPL_TRY(compile_host(e));
  load_spec(e, !e->scene.empty(), (int)e->lay.mgeoms.size());
  if (!e->spec_generic) e->scene.clear();
  e->d_fp = nullptr;
  MJPL_TRY(upload_table(&e->d_ip, e->ip));
  MJPL_TRY(upload_table(&e->d_dp, e->dp));
  std::vector<float> image(e->scene);  // (the scene table in front: a scene-generic library reads backwards from the kernels' table pointer)
  image.insert(image.end(), e->fp.begin(), e->fp.end());
  MJPL_TRY(upload_table(&e->d_fp_base, image));
  e->d_fp = e->d_fp_base + e->scene.size();
  return MJPL_OK;
}

// candidate and distance tables of the pair queries: from the model alone, once, at mjpl_create
int make_pair_tables(mjpl_engine *e) {
  std::vector<int> ip;
  std::vector<double> dp;
  build_contact_table(e, ip, dp);
  e->ct_margin_max = 0.0;
  for (size_t p = 0; p < e->ct_allowed.size(); p++)
    if (!e->ct_allowed[p]) e->ct_margin_max = std::max(e->ct_margin_max, dp[p * CD_LEN + CD_MARGIN]);
  MJPL_TRY(upload_table(&e->d_ct_ip, ip));
  MJPL_TRY(upload_table(&e->d_ct_dp, dp));
  return upload_table(&e->d_dt, build_distance_table(e));
}

// ... and the gradient tables, which follow the planning selection: mjpl_create and mjpl_set_planning
int make_grad_table(mjpl_engine *e) {
  std::vector<double> t;
  MJPL_TRY(build_grad_table(e, t));
  return upload_table(&e->d_gr, t);
}

// ... and the lever table of the certified edge checks, which follows the planning selection and the bounds given:
// mjpl_create, mjpl_set_planning (no bounds), mjpl_sweep_bounds and a mjpl_sweep_edges* call with other bounds
int make_sweep_table(mjpl_engine *e, const double *lo, const double *hi) {
  const size_t nplan = e->qidx.size();
  e->sweep_lo.assign(nplan, -INFINITY);
  e->sweep_hi.assign(nplan, INFINITY);
  if (lo) e->sweep_lo.assign(lo, lo + nplan);
  if (hi) e->sweep_hi.assign(hi, hi + nplan);
  std::vector<double> t(e->sweep_lo);
  t.insert(t.end(), e->sweep_hi.begin(), e->sweep_hi.end());
  const std::vector<double> W = build_sweep_table(e, e->sweep_lo.data(), e->sweep_hi.data());
  t.insert(t.end(), W.begin(), W.end());
  return upload_table(&e->d_sweep_tab, t);
}

size_t lds_bytes(const mjpl_engine *e, int ncolsets, size_t scalar = sizeof(double), int block = kBlock,
                 bool queued = false, size_t colscalar = sizeof(double)) {
  const size_t nplan = e->qidx.size();
  size_t bytes = (((size_t)ncolsets * nplan * block * colscalar + 7) & ~(size_t)7) + (size_t)e->lay.nsave * 7 * block * scalar;
  bytes = (bytes + 7) & ~(size_t)7;
  if (queued)
    bytes += (size_t)(block / 64) * (e->filter_mbox() ? WaveQueue<float, true>::bytes() : WaveQueue<float, false>::bytes()) +
             ((e->fp.size() * sizeof(float) + 7) & ~(size_t)7);
#if MJPL_TABLES_LDS
  bytes += ((e->dp.size() * scalar + 7) / 8) * 8 + ((e->ip.size() * sizeof(int) + 7) / 8) * 8;
#endif
  return bytes ? bytes : 8;
}

// Buffers that share one capacity (uc_cap, llist_cap, item_cap) are all freed before any of them is allocated again.
template <class... B>
int release_all(B &...bufs) {
  int rc = MJPL_OK;
  ((rc = rc != MJPL_OK ? rc : bufs.release()), ...);
  return rc;
}

int uc_reserve(mjpl_engine *e, int64_t n) {
  // MJPL_UC_CAP (create-time, tests): a small hand-over buffer, to exercise its overflow paths
  const size_t want = e->uc_cap_limit ? e->uc_cap_limit : (size_t)std::max<int64_t>(4096, n);
  if (want <= e->uc_cap) return MJPL_OK;
  MJPL_TRY(release_all(e->d_ucq, e->d_ucedge, e->d_ucidx, e->d_ucga, e->d_ucgb));
  e->uc_cap = 0;
  MJPL_TRY(e->d_ucq.reserve(want * std::max<size_t>(1, e->m.nq)));
  MJPL_TRY(e->d_ucedge.reserve(want));
  MJPL_TRY(e->d_ucidx.reserve(want));
  MJPL_TRY(e->d_ucga.reserve(want));
  MJPL_TRY(e->d_ucgb.reserve(want));
  if (!e->d_geomtab) {
    const HostModel &m = e->m;
    std::vector<double> t((size_t)m.ngeom * GTB_LEN, 0.0);
    for (int g = 0; g < m.ngeom; g++) {
      double *r = &t[(size_t)g * GTB_LEN];
      r[GTB_TYPE] = m.geom_type[g];
      for (int k = 0; k < 3; k++) r[GTB_SIZE + k] = m.geom_size[3 * g + k];
      r[GTB_RBOUND] = m.geom_rbound[g];
      r[GTB_MARGIN] = m.geom_margin[g];
      r[GTB_STATIC] = e->lay.geom_static[g] ? 1.0 : 0.0;
      for (int k = 0; k < 3; k++) r[GTB_XPOS + k] = e->lay.st_gxpos[3 * g + k];
      for (int k = 0; k < 9; k++) r[GTB_XMAT + k] = e->lay.st_gxmat[9 * g + k];
    }
    MJPL_TRY(upload_table(&e->d_geomtab, t));
  }
  e->uc_cap = want;
  return MJPL_OK;
}

// where the filter kernels hand single undecided pairs over (uc_reserve first)
UndecidedConfigs undecided(const mjpl_engine *e) {
  UndecidedConfigs uc = {};
  uc.q = e->d_ucq.p; uc.edge = e->d_ucedge.p; uc.idx = e->d_ucidx.p;
  uc.ga = e->d_ucga.p; uc.gb = e->d_ucgb.p;
  uc.count = e->d_ucount + kCtr;
  uc.cap = (int)std::min<size_t>(e->uc_cap, (size_t)1 << 30);
  return uc;
}

int ulist_reserve(mjpl_engine *e, int64_t n) {
  if (!e->d_ucount) {
    // five device counters, each on its own 128-byte line (they are hammered by wave-level atomics
    // of the same kernel: sharing a line costs ~7 % of a step), cleared by one memset per launch:
    //   [0] edge-level undecided list, [kCtr] undecided pairs, [2 kCtr] edges whose endpoint passed,
    //   [3 kCtr] (unused), [4 kCtr] edges left to the walking kernel,
    //   [5 kCtr ..] waypoint items per region, then edges whose endpoint passed per region
    // two sets, used alternately (next_counters): the first kernel of a launch clears the other one
    HIP_TRY(hipMalloc(&e->d_ucount_base, 2 * kNumCtr * kCtr * sizeof(int)));
    HIP_TRY(hipMemset(e->d_ucount_base, 0, 2 * kNumCtr * kCtr * sizeof(int)));
    e->d_ucount = e->d_ucount_base;
    e->d_icount = e->d_ucount + 3 * kCtr;
  }
  return e->d_ulist.reserve((size_t)n);
}

// per-edge scratch of the launches that work from a pool or an item space: walking list, step fractions, claim
// words of the undecided-edge list (cleared when they are made: no generation has claimed anything yet)
int llist_reserve(mjpl_engine *e, int64_t E) {
  if ((size_t)E <= e->llist_cap) return MJPL_OK;
  MJPL_TRY(release_all(e->d_tstep, e->d_llist, e->d_eclaim));
  e->llist_cap = 0;
  MJPL_TRY(e->d_llist.reserve((size_t)E));
  MJPL_TRY(e->d_tstep.reserve((size_t)E));
  MJPL_TRY(e->d_eclaim.reserve((size_t)E));
  HIP_TRY(hipMemsetAsync(e->d_eclaim.p, 0, (size_t)E * sizeof(int), e->stream));
  e->claim_gen = 0;
  e->llist_cap = (size_t)E;
  return MJPL_OK;
}

// a filter launch's generation of the claim words: generations never repeat between clears
int next_claim_gen(mjpl_engine *e) {
  if (++e->claim_gen == std::numeric_limits<int>::max()) {
    HIP_TRY(hipMemsetAsync(e->d_eclaim.p, 0, e->llist_cap * sizeof(int), e->stream));
    e->claim_gen = 1;
  }
  return MJPL_OK;
}

// Raise a kernel's dynamic-LDS limit when a launch needs more than was granted before (per
// device: the attribute belongs to the loaded code object).  Cached: the driver call costs a
// few microseconds, and a step is several launches.
template <class K>
int allow_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) return fail(MJPL_E_CAPACITY, "model needs %zu B of LDS per workgroup (> 160 KiB)", bytes);
  static thread_local std::map<std::pair<const void *, int>, size_t> granted;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  size_t &have = granted[{reinterpret_cast<const void *>(kernel), dev}];
  if (bytes <= have) return MJPL_OK;
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  have = bytes;
  return MJPL_OK;
}

// ---- the two ways a kernel is launched: a kernel of this library on a stream (the engine's, unless the caller names one:
// the look-up's kernels also go to the planner's second) ...
template <class K, class... A>
int launch_kernel(hipStream_t st, K kern, dim3 grid, int block, size_t lds, A... args) {
  MJPL_TRY(allow_lds(kern, lds));
  hipLaunchKernelGGL(kern, grid, dim3(block), lds, st, args...);
  return MJPL_OK;
}

template <class K, class... A>
int launch_kernel(const mjpl_engine *e, K kern, unsigned grid, int block, size_t lds, A... args) {
  return launch_kernel(e->stream, kern, dim3(grid), block, lds, args...);
}

// (a persistent grid: the workgroups that are resident under that LDS grant, or fewer for `ntile` tiles of 64)
template <class K, class... A>
int launch_persistent(const mjpl_engine *e, K kern, size_t lds, long long ntile, A... args) {
  MJPL_TRY(allow_lds(kern, lds));
  hipLaunchKernelGGL(kern, dim3(persistent_grid(kern, lds, ntile)), dim3(kBlock), lds, e->stream, args...);
  return MJPL_OK;
}

// (a pool kernel of mjpl_fused.h: fused_launch sizes the grid)
template <class K>
int launch_pool(const mjpl_engine *e, K kern, int nwaves, size_t lds, const FusedArgs &fa, const char *what) {
  MJPL_TRY(allow_lds(kern, lds));
  return fused_launch(kern, nwaves, lds, fa, e->stream) == hipSuccess ? MJPL_OK : fail(MJPL_E_HIP, "the %s kernel failed to launch", what);
}

// ... or the entry point of a model's library, which answers non-zero when its launch failed
int spec_rc(int launched, const char *what) {
  return launched == 0 ? MJPL_OK : fail(MJPL_E_HIP, "specialised %s kernel failed to launch", what);
}

// Can this engine's edge launches run the fused filter kernel (mjpl_fused.h), and how: waves per workgroup
// (twelve = one workgroup per CU at three waves per SIMD; four for the one-wave-per-SIMD build of models with
// moving boxes), entries of a workgroup's pool (what the CU's LDS leaves, at least 64 per wave: one endpoint tile
// each) and the dynamic LDS of a workgroup.  `spec`: the library that would launch it (the engine's own, or its
// certificate build).
bool fused_plan(const mjpl_engine *e, const SpecLib *spec, int *nwaves, size_t *lds, int *ring) {
  if (!e->fused || !e->filter || !e->fb.usable || !e->two_pass || !e->expand || e->immediate()) return false;
  const int nplan = (int)e->qidx.size();
  const bool mbox = e->filter_mbox();
  // (models with moving boxes run one wave per SIMD: four waves per workgroup, and measured 5 % SLOWER fused than as the
  // two kernels -- 1.63 vs 1.55 ms on Franka-P with the ten pad boxes; MJPL_FUSED_MBOX=1 runs them fused all the same)
  if (mbox && !e->fused_mbox && !spec) return false;
  if (!fused_fits(nplan, e->lay.nsave, mbox)) return false;
  const int nw = spec ? spec->fused_waves : (mbox ? 4 : kFusedWaves);
  const size_t budget = (size_t)160 * 1024;
  const bool cert = spec && spec->fused_cert;
  const size_t base = fused_lds_bytes(nw, nplan, e->lay.nsave, e->fp.size(), mbox, 0, cert);
  if (base + (size_t)(64 * nw + 64) * kFusedEntryBytes > budget) return false;
  int r = (int)std::min<size_t>(kFusedMaxPool, (budget - base) / kFusedEntryBytes / 64 * 64);
  if (e->fused_pool_cap > 0) r = std::max(64 * nw + 64, std::min(r, e->fused_pool_cap / 64 * 64));  // (tests: a ring that wraps)
  *nwaves = nw;
  *lds = fused_lds_bytes(nw, nplan, e->lay.nsave, e->fp.size(), mbox, r, cert);
  *ring = r;
  return true;
}

// ... and with the filter off: the float64 checks through the same pool (k_edges_fused_f64)
bool fused_f64_ok(const mjpl_engine *e) {
  return e->fused && e->two_pass && e->expand &&
         fused_f64_lds_bytes(kFusedF64Waves, (int)e->qidx.size(), e->lay.nsave, 64 * kFusedF64Waves + 64) <= (size_t)160 * 1024;
}

// ---- What one edge launch will do, decided before anything is reserved or enqueued (no HIP call in here).
// mjpl_get_info reports from the same function what a launch WOULD do.
//   kFused      the binary32 filter as ONE kernel (k_edges_fused): endpoint and waypoint tiles from a pool in LDS
//   kTwoKernel  endpoint kernel, then (expand) the item kernel over the waypoints it emitted; ordinary or persistent grids
//   kOnePass    the walking kernel alone (one pass asked for, or only the interior)
//   kF64Pool    filter off: the float64 checks through the pool (k_edges_fused_f64), then k_check_edges over the walking list
//   kExact      filter off: k_check_edges is the whole launch
// The first three are the filter's; behind them comes either k_tail (`tail`: walking role, pair re-check and exact
// edge role in one launch) or the walking kernel, the pair re-check and k_check_edges over the undecided edges.
enum class EdgePipe { kFused, kTwoKernel, kOnePass, kF64Pool, kExact };

struct EdgePlan {
  EdgePipe pipe;
  bool two_pass;    // endpoints of all edges, then the interior of the edges whose endpoint passed (unless only the interior was asked for)
  // interior waypoints: one lane per waypoint for ordinary edges (the endpoint kernel emits the waypoints as items),
  // the walking kernel for long edges and for models with moving boxes
  bool expand;
  // endpoint and item kernels as persistent grids (one wave per tile of 64, tiles from a device counter): the default
  // for the queued interpreter when the interior waypoints become items
  bool persistent;
  bool tail;        // everything behind the item pass in one launch (k_tail)
  int single;       // fused: a batch that leaves most of the chip idle takes one round of checks, not two (the endpoint as an item)
  // fused: the library that launches it, null for the interpreting kernel (a big batch goes to the model's certificate
  // build, if the engine found one beside the program's own library: load_spec)
  const SpecLib *flib;
  // float64 pool: the check through the candidate queues (narrowphase with full lanes) where the model has the queued
  // build's shape and eight waves' queues fit beside the rows and a pool, else the immediate interpreter
  // (MJPL_F64_QUEUED=0); generated: the library's straight-line check (ExactFull) is tried first (MJPL_F64_SPEC=0: never)
  bool queued, generated;
  unsigned grid, fgrid;  // exact kernels (kBlock threads), filter kernels (fblock threads)
  int fblock;
  size_t lds_exact;
  size_t lds_walk;       // walking kernel: float64 columns
  size_t lds_items;      // endpoint and item kernels of the queued interpreter keep binary32 columns
  size_t lds_endpoints;  // ... the immediate interpreter's endpoint kernel walks the waypoint recurrence in a second column set
  size_t lds_persistent, lds_tail, lds_pool;
  int fwaves, pool;      // fused / float64 pool: waves per workgroup, entries of a workgroup's pool (0: neither kernel runs)
};

EdgePlan plan_edges(const mjpl_engine *e, int64_t E, int flags, bool long_edges) {
  EdgePlan p = {};
  const bool imm = e->immediate();
  const int nplan = (int)e->qidx.size();
  p.grid = (unsigned)((E + kBlock - 1) / kBlock);
  p.fblock = imm ? kBlock : kFilterBlock;
  p.fgrid = (unsigned)((E + p.fblock - 1) / p.fblock);
  p.lds_exact = lds_bytes(e, 1);
  p.lds_walk = lds_bytes(e, 1, sizeof(float), p.fblock, !imm);
  p.lds_items = lds_bytes(e, 1, sizeof(float), p.fblock, !imm, imm ? sizeof(double) : sizeof(float));
  p.lds_endpoints = imm ? lds_bytes(e, 2, sizeof(float), p.fblock, false) : p.lds_items;
  p.lds_persistent = persistent_lds_bytes(nplan, e->lay.nsave, e->fp.size(), e->filter_mbox());
  p.lds_tail = std::max(p.lds_walk, p.lds_exact);
  p.two_pass = e->two_pass && !(flags & MJPL_EDGE_INTERIOR_ONLY);
  p.expand = p.two_pass && e->expand;
  p.persistent = (e->persist < 0 ? e->spec != nullptr : e->persist != 0) && p.expand && !imm;
  p.tail = p.expand && e->fused_tail && !imm;
  p.single = (E <= (int64_t)e->fused_single_max) ? 1 : 0;
  p.flib = (e->spec && !e->spec_generic && e->spec_cert && e->fused_cert && e->fused_cert_min_edges > 0 && E >= e->fused_cert_min_edges &&
            E > (int64_t)e->fused_single_max) ? e->spec_cert : e->spec;
  if (e->filter && e->fb.usable && E < (int64_t)1 << 29) {  // item ids travel in 29 bits of the per-lane flag words
    // (long_edges: the batch holds a few long edges -> the kernels with checkpoints, see mjpl_check_edges)
    if (p.expand && !long_edges && fused_plan(e, p.flib, &p.fwaves, &p.lds_pool, &p.pool)) p.pipe = EdgePipe::kFused;
    else p.pipe = p.two_pass ? EdgePipe::kTwoKernel : EdgePipe::kOnePass;
  } else if (fused_f64_ok(e) && !(flags & MJPL_EDGE_INTERIOR_ONLY) && E < (int64_t)1 << 30) {
    p.pipe = EdgePipe::kF64Pool;
    p.fwaves = kFusedF64Waves;
    p.queued = e->f64_queued && !e->exact_general() &&
               fused_f64_lds_bytes(kFusedF64Waves, nplan, e->lay.nsave, 64 * kFusedF64Waves + 64, true) <= (size_t)160 * 1024;
    p.generated = p.queued && e->spec && e->spec->fused_f64 && e->f64_spec && e->spec->generic_rows == 0;
    const size_t base = fused_f64_lds_bytes(kFusedF64Waves, nplan, e->lay.nsave, 0, p.queued);
    p.pool = (int)std::min<size_t>(kFusedMaxPool, ((size_t)160 * 1024 - base) / kFusedEntryBytes / 64 * 64);
    if (e->fused_pool_cap > 0) p.pool = std::max(64 * kFusedF64Waves + 64, std::min(p.pool, e->fused_pool_cap / 64 * 64));
    p.lds_pool = fused_f64_lds_bytes(kFusedF64Waves, nplan, e->lay.nsave, p.pool, p.queued);
  } else {
    p.pipe = EdgePipe::kExact;
  }
  return p;
}

// A filter launch takes the cleared counter set and returns the other one, which its first kernel is
// to clear for the launch after it.
int *next_counters(mjpl_engine *e) {
  if (e->counters_stale) {  // a launch failed between taking its set and its first kernel
    (void)hipMemsetAsync(e->d_ucount_base, 0, 2 * (size_t)kNumCtr * kCtr * sizeof(int), e->stream);
    e->counters_stale = false;
  }
  int *other = e->d_ucount;
  e->d_ucount = (e->d_ucount == e->d_ucount_base) ? e->d_ucount_base + (size_t)kNumCtr * kCtr : e->d_ucount_base;
  e->d_icount = e->d_ucount + 3 * kCtr;
  return other;
}

// pick the <MAXS, WBOX, MBOX> instantiation of the EXACT kernels for this model
template <class F>
int dispatch_variant(const mjpl_engine *e, F &&f) {
  if (e->exact_general()) return f(std::integral_constant<int, 32>{}, std::true_type{}, std::true_type{});
  auto with_box = [&](auto S) -> int {
    if (e->lay.wbox) return f(S, std::true_type{}, std::false_type{});
    return f(S, std::false_type{}, std::false_type{});
  };
  switch (e->lay.maxs) {
    case 4: return with_box(std::integral_constant<int, 4>{});
    case 8: return with_box(std::integral_constant<int, 8>{});
    case 16: return with_box(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 32>{}, std::true_type{}, std::true_type{});
  }
}

// ... and of the FILTER kernels
template <class F>
int dispatch_filter(const mjpl_engine *e, F &&f) {
  if (e->immediate()) return f(std::integral_constant<int, 32>{}, std::true_type{}, std::true_type{});
  if (e->filter_mbox()) return f(std::integral_constant<int, kQueuedMaxSlots>{}, std::true_type{}, std::true_type{});
  return dispatch_variant(e, f);
}

// option "kernel_timer": an event on either side of the launches of class `mode`
void kt_mark(mjpl_engine *e, int mode, hipStream_t st) {
  if (!(e->kt_mode & mode)) return;
  const int c = mode == 2 ? 1 : 0;
  if (e->kt_used[c] + 1 > (int)e->kt_ev[c].size()) {
    if (e->kt_ev[c].size() >= 4096) return;  // (a run of more launches than that: the later ones go untimed)
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) return;
    e->kt_ev[c].push_back(ev);
  }
  (void)hipEventRecord(e->kt_ev[c][(size_t)e->kt_used[c]++], st);
}

struct KtScope {  // ... around everything a scope enqueues on the engine's stream
  mjpl_engine *e; int mode;
  KtScope(mjpl_engine *e_, int mode_) : e(e_), mode(mode_) { kt_mark(e, mode, e->stream); }
  ~KtScope() { kt_mark(e, mode, e->stream); }
};

// exact re-check of the undecided pairs: the model's own straight-line float64 FK if it has a library.  The grid is
// sized for a generous share of the batch; surplus blocks return at once.
int launch_patch(mjpl_engine *e, const UndecidedConfigs &uc, uint8_t *dvalid, int32_t *dfb) {
  const unsigned pgrid = (unsigned)std::min<size_t>((uc.cap + kBlock - 1) / kBlock, 1024);
  const size_t ldsc = lds_bytes(e, 1);
  const GeomTable gt = {e->d_geomtab, e->lay.moving_base()};
  if (e->spec)
    return spec_rc(e->spec->patch(e->stream, pgrid, (unsigned)kBlock, ldsc, e->d_ip, (int)e->ip.size(), e->d_dp, (int)e->dp.size(), gt, uc, dvalid,
                                  dfb), "pair");
  return launch_kernel(e, k_patch_pairs<void>, pgrid, kBlock, ldsc, e->d_ip, (int)e->ip.size(), e->d_dp, (int)e->dp.size(), gt, uc, dvalid, dfb);
}

struct CounterGuard {  // marks the counter sets for a full clear unless the launch got through
  mjpl_engine *e;
  bool armed;
  ~CounterGuard() { if (armed) e->counters_stale = true; }
};

int launch_configs(mjpl_engine *e, const double *dQ, int64_t N, int layout, uint8_t *dvalid,
                   unsigned long long *dbits) {
  if (N == 0) return MJPL_OK;
  const int nip = (int)e->ip.size(), nfp = (int)e->fp.size(), ndp = (int)e->dp.size();
  const bool filter = e->filter && e->fb.usable && dvalid && !dbits && N < (int64_t)1 << 29;
  if (filter) {
    MJPL_TRY(ulist_reserve(e, N));
    int *zero_next = next_counters(e);
    CounterGuard guard{e, true};
    MJPL_TRY(uc_reserve(e, N));  // (both interpreters hand single undecided pairs over)
    const UndecidedConfigs uc = undecided(e);
    const int fblock = e->immediate() ? kBlock : kFilterBlock;
    const unsigned fgrid = (unsigned)((N + fblock - 1) / fblock);
    // (queued interpreter: binary32 columns; the immediate one: float64 columns)
    const size_t lds_filter = lds_bytes(e, 1, sizeof(float), fblock, !e->immediate(), e->immediate() ? sizeof(double) : sizeof(float));
    kt_mark(e, 1, e->stream);
    const int rc = e->spec
        ? spec_rc(e->spec->configs(e->stream, fgrid, (unsigned)fblock, lds_filter, e->d_ip, nip, e->d_fp, nfp, dQ, N, layout, e->fb.tol,
                                   dvalid, e->d_ulist.p, e->d_ucount, uc, zero_next), "configuration")
        : dispatch_filter(e, [&](auto S, auto W, auto M) -> int {
            return launch_kernel(e, k_filter_configs<void, S(), W(), M()>, fgrid, fblock, lds_filter, e->d_ip, nip, e->d_fp, nfp, dQ, N, layout,
                                 e->fb.tol, dvalid, e->d_ulist.p, e->d_ucount, uc, zero_next);
          });
    kt_mark(e, 1, e->stream);
    MJPL_TRY(rc);
    guard.armed = false;
    MJPL_TRY(launch_patch(e, uc, dvalid, nullptr));  // the undecided pairs; rows here are planning columns, AoS
  }
  const unsigned grid = (unsigned)((N + kBlock - 1) / kBlock);
  MJPL_TRY(dispatch_variant(e, [&](auto S, auto W, auto M) -> int {
    return launch_kernel(e, k_check_configs<S(), W(), M()>, grid, kBlock, lds_bytes(e, 1), e->d_ip, nip, e->d_dp, ndp, dQ, N, layout, dvalid, dbits,
                         filter ? (const int *)e->d_ulist.p : nullptr, filter ? (const int *)e->d_ucount : nullptr, UndecidedConfigs{},
                         (int32_t *)nullptr);
  }));
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// ---- one edge launch: the batch as the caller gave it, and a function per stage of the pipelines of plan_edges

struct EdgeBatch {
  const double *QA, *QB; int64_t E; double step; int layout, flags;
  uint8_t *valid; int32_t *first_bad;
};

// What FusedArgs and TailArgs have in common: the batch, the program, the walking list -- and, with `uc`, the filter's
// side of a launch (binary32 tables, tolerance, both undecided lists), which the float64 pool launch leaves zero.
template <class A>
A batch_args(const mjpl_engine *e, const EdgeBatch &b, const UndecidedConfigs *uc) {
  A a = {};
  a.ip = e->d_ip; a.nip = (int)e->ip.size();
  a.QA = b.QA; a.QB = b.QB; a.E = (long long)b.E; a.layout = b.layout; a.step = b.step;
  a.valid = b.valid; a.first_bad = b.first_bad;
  a.status = e->d_status;
  a.llist = e->d_llist.p; a.lcount = e->d_icount + kCtr;
  if (uc) {
    a.fp = e->d_fp; a.nfp = (int)e->fp.size();
    a.tol = e->fb.tol;
    a.uc = *uc;
    a.ulist = e->d_ulist.p; a.ucount = e->d_ucount;
  }
  return a;
}

// ... and the two pool kernels: statistics, the counter set to clear, pool and policy
FusedArgs pool_args(const mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, const UndecidedConfigs *uc, int *zero_next) {
  FusedArgs fa = batch_args<FusedArgs>(e, b, uc);
  fa.item_count = e->d_ucount + 5 * kCtr;
  fa.surv_count = e->d_ucount + (5 + kItemRegions) * kCtr;
  fa.cert_count = e->d_ucount + (size_t)kCtrCertified * kCtr;
  fa.zero_next = zero_next;
  fa.pool = p.pool; fa.policy = e->fused_policy;
  return fa;
}

// kFused: ONE filter kernel for the launch (mjpl_fused.h), endpoint tiles and waypoint tiles from one work pool
int stage_fused(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, const UndecidedConfigs &uc, int *zero_next) {
  FusedArgs fa = pool_args(e, p, b, &uc, zero_next);
  fa.claim = e->d_eclaim.p; fa.gen = e->claim_gen;
  fa.tstep = e->d_tstep.p;
  fa.cert = e->fused_cert;
  fa.kmax = e->fused_kmax;
  fa.single = p.single;
  if (e->fused_dbg_path) {  // diagnostic runs: per-wave counters of the most recent launch, written out at mjpl_destroy
    MJPL_TRY(e->d_fused_dbg.reserve(kFusedDbgWaves * 8));
    HIP_TRY(hipMemsetAsync(e->d_fused_dbg.p, 0, kFusedDbgWaves * 8 * sizeof(unsigned long long), e->stream));
    fa.dbg = e->d_fused_dbg.p;
  }
  if (p.flib) return spec_rc(p.flib->fused(e->stream, p.fwaves, p.lds_pool, fa), "fused");
  return dispatch_filter(e, [&](auto S, auto W, auto M) -> int {
    if constexpr (S() <= kQueuedMaxSlots) {
      constexpr int NW = M() ? 4 : kFusedWaves;
      if (p.fwaves != NW) return fail(MJPL_E_ARG, "fused kernel: %d waves per workgroup asked for, this build has %d", p.fwaves, NW);
      return launch_pool(e, k_edges_fused<void, S(), W(), M(), NW>, NW, p.lds_pool, fa, "fused");
    } else {
      return fail(MJPL_E_ARG, "the fused kernel serves the queued interpreter");
    }
  });
}

// kTwoKernel with expand: the item space of the launch.  Room for 8 waypoints per edge on average, and never less
// than a quarter of a million items: a handful of long edges (path shortcutting) is best served one waypoint per
// lane, too
int items_reserve(mjpl_engine *e, const EdgePlan &p, int64_t E, ItemBuffers *ib) {
  size_t want = std::min<size_t>(std::max<size_t>((size_t)E * 8, (size_t)1 << 18) + 4096, e->item_cap_limit);
  want = (want + p.fblock - 1) / p.fblock * p.fblock;  // whole blocks (the item space is split into regions of them)
  if (want > e->item_cap) {
    MJPL_TRY(release_all(e->d_itemedge, e->d_itemidx));
    e->item_cap = 0;
    MJPL_TRY(e->d_itemedge.reserve(want));
    MJPL_TRY(e->d_itemidx.reserve(want));
    e->item_cap = want;
  }
  const int kmax = (int)std::min<size_t>(std::max<size_t>(e->item_cap / (size_t)E, kExpandMinWaypoints), 1 << 16);
  double *ckpt = nullptr;
  if (kmax >= kCkptEvery) {
    // checkpoint rows, made by the first launch with long items: one per item slot, sized by nq, the upper bound of
    // nplan (mjpl_set_planning may widen the planning set)
    MJPL_TRY(e->d_itemck.reserve(e->item_cap * std::max<size_t>(1, e->m.nq)));
    ckpt = e->d_itemck.p;
  }
  // regions: enough workgroups behind each counter to fill it evenly, few enough waves to not queue up
  const int regions = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(kItemRegions, p.fgrid / 8), e->item_cap / p.fblock));
  const int regcap = (int)(e->item_cap / regions / p.fblock * p.fblock);
  *ib = ItemBuffers{e->d_itemedge.p, e->d_itemidx.p, e->d_ucount + 5 * kCtr, regions * regcap, regions, regcap,
                    e->d_ucount + (5 + kItemRegions) * kCtr, e->d_llist.p,
                    e->d_icount + kCtr, kmax, e->d_tstep.p, ckpt, e->d_eclaim.p, e->claim_gen};
  return MJPL_OK;
}

// kTwoKernel: endpoints of all edges; the survivors go to d_slist, or (expand) their waypoints to the item space
int stage_endpoints(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, const UndecidedConfigs &uc, const ItemBuffers &ib,
                    int *zero_next) {
  const int nip = (int)e->ip.size(), nfp = (int)e->fp.size();
  int *scount = e->d_ucount + 2 * kCtr, *etiles = e->d_ucount + kCtrEndpointTiles * kCtr;
  if (p.persistent && e->spec)
    return spec_rc(e->spec->endpoints_pw(e->stream, p.lds_persistent, e->d_ip, nip, e->d_fp, nfp, b.QA, b.QB, b.E, b.layout, e->fb.tol, b.valid,
                                         b.first_bad, e->d_status, e->d_ulist.p, e->d_ucount, uc, ib, b.step, zero_next, etiles), "endpoint");
  if (p.persistent)
    return dispatch_filter(e, [&](auto S, auto W, auto M) -> int {
      if constexpr (S() <= kQueuedMaxSlots) {
        return launch_persistent(e, k_filter_endpoints_pw<void, S(), W(), M()>, p.lds_persistent, (b.E + 63) / 64, e->d_ip, nip, e->d_fp, nfp, b.QA,
                                 b.QB, b.E, b.layout, e->fb.tol, b.valid, b.first_bad, e->d_status, e->d_ulist.p, e->d_ucount, uc, ib, b.step,
                                 zero_next, etiles);
      } else {
        return fail(MJPL_E_ARG, "persistent kernels serve the queued interpreter");
      }
    });
  if (e->spec)
    return spec_rc(e->spec->endpoints(e->stream, p.fgrid, (unsigned)p.fblock, p.lds_endpoints, e->d_ip, nip, e->d_fp, nfp, b.QA, b.QB, b.E, b.layout,
                                      e->fb.tol, b.valid, b.first_bad, e->d_status, e->d_ulist.p, e->d_ucount, uc, e->d_slist.p, scount, ib,
                                      b.step, zero_next), "endpoint");
  return dispatch_filter(e, [&](auto S, auto W, auto M) -> int {
    return launch_kernel(e, k_filter_endpoints<void, S(), W(), M()>, p.fgrid, p.fblock, p.lds_endpoints, e->d_ip, nip, e->d_fp, nfp, b.QA, b.QB, b.E,
                         b.layout, e->fb.tol, b.valid, b.first_bad, e->d_status, e->d_ulist.p, e->d_ucount, uc, e->d_slist.p, scount, ib, b.step,
                         zero_next);
  });
}

// kTwoKernel with expand: one lane per waypoint item
int stage_items(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, const UndecidedConfigs &uc, const ItemBuffers &ib) {
  const int nip = (int)e->ip.size(), nfp = (int)e->fp.size();
  const unsigned igrid = (unsigned)(ib.cap / p.fblock);  // (regions of whole blocks)
  const EdgeSource src = {b.QA, b.QB, (long long)b.E, b.layout, b.step, ib.ckpt};
  int *itiles = e->d_ucount + kCtrItemTiles * kCtr;
  if (p.persistent && e->spec)
    return spec_rc(e->spec->items_pw(e->stream, p.lds_persistent, e->d_ip, nip, e->d_fp, nfp, ib, src, e->fb.tol, b.valid, b.first_bad,
                                     e->d_ulist.p, e->d_ucount, uc, itiles), "item");
  if (p.persistent)
    return dispatch_filter(e, [&](auto S, auto W, auto M) -> int {
      if constexpr (S() <= kQueuedMaxSlots) {
        return launch_persistent(e, k_filter_items_pw<void, S(), W(), M()>, p.lds_persistent, (long long)ib.cap / 64, e->d_ip, nip, e->d_fp, nfp, ib,
                                 src, e->fb.tol, b.valid, b.first_bad, e->d_ulist.p, e->d_ucount, uc, itiles);
      } else {
        return fail(MJPL_E_ARG, "persistent kernels serve the queued interpreter");
      }
    });
  if (e->spec)
    return spec_rc(e->spec->items(e->stream, igrid, (unsigned)p.fblock, p.lds_items, e->d_ip, nip, e->d_fp, nfp, ib, src, e->fb.tol, b.valid,
                                  b.first_bad, e->d_ulist.p, e->d_ucount, uc), "item");
  return dispatch_filter(e, [&](auto S, auto W, auto M) -> int {
    return launch_kernel(e, k_filter_items<void, S(), W(), M()>, igrid, p.fblock, p.lds_items, e->d_ip, nip, e->d_fp, nfp, ib, src, e->fb.tol,
                         b.valid, b.first_bad, e->d_ulist.p, e->d_ucount, uc);
  });
}

// everything behind the item pass in one launch: walking role over the long-edge list, pair
// re-check, exact edge role over the undecided-edge list (k_tail)
int stage_tail(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, const UndecidedConfigs &uc) {
  TailArgs ta = batch_args<TailArgs>(e, b, &uc);
  ta.dp = e->d_dp; ta.ndp = (int)e->dp.size();
  ta.gt = GeomTable{e->d_geomtab, e->lay.moving_base()};
  ta.flags = b.flags;
  ta.done = e->d_ucount + kCtrTailDone * kCtr;
  ta.nw = ta.nx = (int)std::min<int64_t>((b.E + kBlock - 1) / kBlock, 64);
  ta.np = (int)std::min<size_t>((uc.cap + kBlock - 1) / kBlock, 64);
  if (e->spec) return spec_rc(e->spec->tail(e->stream, p.lds_tail, ta), "tail");
  auto go = [&](auto SF, auto SD, auto W, auto M) -> int {
    return launch_kernel(e, k_tail<void, SF(), SD(), W(), M()>, (unsigned)(ta.nw + ta.np + ta.nx), kBlock, p.lds_tail, ta);
  };
  if (e->exact_general())  // (moving boxes: 24-slot queued filter build, general exact build)
    return go(std::integral_constant<int, kQueuedMaxSlots>{}, std::integral_constant<int, 32>{}, std::true_type{}, std::true_type{});
  return dispatch_variant(e, [&](auto S, auto W, auto M) -> int { return go(S, S, W, M); });
}

// the walking kernel (k_filter_edges) over `rlist`: every edge in a one-pass launch (null list), which is then the
// launch's first kernel and clears the other counter set
int stage_walk(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, const UndecidedConfigs &uc, const int *rlist, const int *rcount,
               int *zero_next) {
  return dispatch_filter(e, [&](auto S, auto W, auto M) -> int {
    return launch_kernel(e, k_filter_edges<S(), W(), M()>, p.fgrid, p.fblock, p.lds_walk, e->d_ip, (int)e->ip.size(), e->d_fp, (int)e->fp.size(),
                         b.QA, b.QB, b.E, b.step, b.layout, p.two_pass ? (b.flags | MJPL_EDGE_INTERIOR_ONLY) : b.flags, e->fb.tol, b.valid,
                         b.first_bad, e->d_status, e->d_ulist.p, e->d_ucount, uc, rlist, rcount, p.two_pass ? (int *)nullptr : zero_next);
  });
}

// undecided waypoints: the exact configuration kernel in patch mode for the whole configurations the immediate
// filter hands over (entries with ga < 0), then the single geom pairs (entries with ga >= 0)
int stage_patch(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, const UndecidedConfigs &uc) {
  if (e->immediate()) {
    const unsigned pgrid = (unsigned)std::min<size_t>((uc.cap + kBlock - 1) / kBlock, 1024);
    MJPL_TRY(dispatch_variant(e, [&](auto S, auto W, auto M) -> int {
      return launch_kernel(e, k_check_configs<S(), W(), M()>, pgrid, kBlock, p.lds_exact, e->d_ip, (int)e->ip.size(), e->d_dp, (int)e->dp.size(),
                           (const double *)uc.q, (int64_t)0, (int)MJPL_AOS, b.valid, (unsigned long long *)nullptr, (const int *)nullptr,
                           (const int *)nullptr, uc, b.first_bad);
    }));
  }
  return launch_patch(e, uc, b.valid, b.first_bad);
}

// kF64Pool: endpoints, then the interior waypoints of the survivors as items; edges of more than kFusedF64Kmax
// waypoints are left on the walking list
int stage_pool_f64(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, int *zero_next) {
  FusedArgs fa = pool_args(e, p, b, nullptr, zero_next);
  fa.dp = e->d_dp; fa.ndp = (int)e->dp.size();
  fa.kmax = kFusedF64Kmax;
  if (p.generated) {
    const int r = e->spec->fused_f64(e->stream, kFusedF64Waves, p.lds_pool, fa);
    if (r == 0) return MJPL_OK;
    if (r != -1) return fail(MJPL_E_HIP, "the generated float64 pool kernel failed to launch");  // (-1: refused, the interpreting kernel runs)
  }
  return dispatch_variant(e, [&](auto S, auto W, auto M) -> int {
    if constexpr (!M() && S() <= 16) {
      if (p.queued)
        return launch_pool(e, k_edges_fused_f64<S(), W(), false, kFusedF64Waves, true>, kFusedF64Waves, p.lds_pool, fa, "float64 pool");
    }
    return launch_pool(e, k_edges_fused_f64<S(), W(), M(), kFusedF64Waves, false>, kFusedF64Waves, p.lds_pool, fa, "float64 pool");
  });
}

// k_check_edges, the exact kernel: over the edges of `list` (the undecided edges of a filter launch; the walking list
// of the float64 pool, interior waypoints only: the endpoint's verdict stands), or over the whole batch (null)
int stage_exact(mjpl_engine *e, const EdgePlan &p, const EdgeBatch &b, int flags, const int *list, const int *count) {
  return dispatch_variant(e, [&](auto S, auto W, auto M) -> int {
    return launch_kernel(e, k_check_edges<S(), W(), M()>, p.grid, kBlock, p.lds_exact, e->d_ip, (int)e->ip.size(), e->d_dp, (int)e->dp.size(), b.QA,
                         b.QB, b.E, b.step, b.layout, flags, b.valid, b.first_bad, e->d_status, list, count);
  });
}

// stages of one edge launch, in stream order (include/mjpl_hip.h: MJPL_STAGE_*)
#define MJPL_MARK(k)                                                          \
  do {                                                                        \
    if (e->marks) HIP_TRY(hipEventRecord(e->marks[k], e->stream));            \
  } while (0)

// One edge launch.  What runs between the marks, per pipeline (plan_edges):
//   kFused       0  k_edges_fused                        1  2 |  with the tail:  3  k_tail  4  5
//   kTwoKernel   0  endpoints  1  items (expand)            2 |  without:        walk  3  patch  4  k_check_edges  5
//   kOnePass     0             1                            2 |  (never the tail)
//   kF64Pool     0  k_edges_fused_f64  1  2  3  4  k_check_edges over the walking list  5
//   kExact       0  1  2  3  4  k_check_edges  5
// Of the two counter sets a launch works in the cleared one; its first kernel clears the other (zero_next), and from
// then on the guard stands down: the sets are in step again.
int launch_edges(mjpl_engine *e, const double *dQA, const double *dQB, int64_t E, double step,
                 int layout, int flags, uint8_t *dvalid, int32_t *dfb, bool long_edges) {
  if (E == 0) return MJPL_OK;
  const EdgePlan p = plan_edges(e, E, flags, long_edges);
  const EdgeBatch b = {dQA, dQB, E, step, layout, flags, dvalid, dfb};
  if (p.pipe == EdgePipe::kExact) {
    for (int k = 0; k <= 4; k++) MJPL_MARK(k);
    MJPL_TRY(stage_exact(e, p, b, flags, nullptr, nullptr));
  } else if (p.pipe == EdgePipe::kF64Pool) {
    MJPL_TRY(ulist_reserve(e, E));
    MJPL_TRY(llist_reserve(e, E));
    int *zero_next = next_counters(e);
    CounterGuard guard{e, true};
    MJPL_MARK(0);
    MJPL_TRY(stage_pool_f64(e, p, b, zero_next));
    guard.armed = false;
    for (int k = 1; k <= 4; k++) MJPL_MARK(k);
    MJPL_TRY(stage_exact(e, p, b, flags | MJPL_EDGE_INTERIOR_ONLY, e->d_llist.p, e->d_icount + kCtr));
  } else {
    MJPL_TRY(ulist_reserve(e, E));
    MJPL_TRY(uc_reserve(e, E));
    int *zero_next = next_counters(e);  // (this launch's own set was cleared by the launch before it)
    CounterGuard guard{e, true};
    const UndecidedConfigs uc = undecided(e);
    MJPL_MARK(0);
    if (p.expand) {
      MJPL_TRY(llist_reserve(e, E));
      MJPL_TRY(next_claim_gen(e));
    }
    const int *rlist = nullptr, *rcount = nullptr;  // work list of the walking kernel: all edges, ...
    ItemBuffers ib = {};
    if (p.pipe == EdgePipe::kFused) {
      MJPL_TRY(stage_fused(e, p, b, uc, zero_next));
      guard.armed = false;
    } else {
      if (p.expand) MJPL_TRY(items_reserve(e, p, E, &ib));
      if (p.two_pass) {
        MJPL_TRY(e->d_slist.reserve((size_t)E));
        MJPL_TRY(stage_endpoints(e, p, b, uc, ib, zero_next));
        guard.armed = false;
        rlist = e->d_slist.p;  // ... those whose endpoint passed, ...
        rcount = e->d_ucount + 2 * kCtr;
      }
    }
    MJPL_MARK(1);
    if (p.expand) {
      if (p.pipe != EdgePipe::kFused) MJPL_TRY(stage_items(e, p, b, uc, ib));
      rlist = e->d_llist.p;  // ... or what the pool or the item space left to it
      rcount = e->d_icount + kCtr;
    }
    MJPL_MARK(2);
    if (p.tail) {
      MJPL_MARK(3);
      MJPL_TRY(stage_tail(e, p, b, uc));
      guard.armed = false;
      MJPL_MARK(4);
    } else {
      MJPL_TRY(stage_walk(e, p, b, uc, rlist, rcount, zero_next));
      guard.armed = false;
      MJPL_MARK(3);
      MJPL_TRY(stage_patch(e, p, b, uc));
      MJPL_MARK(4);
      MJPL_TRY(stage_exact(e, p, b, flags, e->d_ulist.p, e->d_ucount));
    }
  }
  MJPL_MARK(5);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// Every pair query refuses a model whose candidate table holds a pair no routine here handles.
int check_pair_types(const mjpl_engine *e) {
  if (e->ct_unsupported < 0) return MJPL_OK;
  const int g1 = e->ct_g1[e->ct_unsupported], g2 = e->ct_g2[e->ct_unsupported];
  return fail(MJPL_E_PAIRTYPE, "candidate pair (%d, %d) has geom types (%d, %d): no pair routine here handles it", g1,
              g2, e->m.geom_type[g1], e->m.geom_type[g2]);
}

// Rows per launch of a pair-query kernel (min(N, kContactRows)), its dynamic LDS and its FK scratch rows:
// gx [rows][ngeom][3], gm [rows][ngeom][9]
struct PairLaunch {
  int64_t rows;
  size_t lds;
  double *gx, *gm;
};

// What every pair-query launch needs first: the pair-type check, the FK scratch and the kernel's LDS grant.
template <class K>
int pair_query_prologue(mjpl_engine *e, K kernel, int64_t N, PairLaunch *pl, int ncolsets = 1) {
  int rc = check_pair_types(e);
  if (rc != MJPL_OK) return rc;
  const size_t ng = e->m.ngeom;
  pl->rows = std::min<int64_t>(N, kContactRows);
  rc = e->d_ct_scratch.reserve((size_t)pl->rows * ng * 12);
  if (rc != MJPL_OK) return rc;
  pl->gx = e->d_ct_scratch.p;
  pl->gm = e->d_ct_scratch.p + (size_t)pl->rows * ng * 3;
  pl->lds = lds_bytes(e, ncolsets);
  return allow_lds(kernel, pl->lds);
}

// One k_contacts launch per kContactRows configurations (the FK scratch holds that many rows).
int launch_contacts(mjpl_engine *e, const double *dQ, int64_t N, int layout, unsigned long long *dbits) {
  const int P = (int)e->ct_g1.size();
  const int W = (P + 63) / 64;
  if (N == 0 || P == 0) return MJPL_OK;
  PairLaunch pl;
  int rc = pair_query_prologue(e, k_contacts, N, &pl);
  if (rc != MJPL_OK) return rc;
  for (int64_t i0 = 0; i0 < N; i0 += pl.rows) {
    const int64_t n = std::min<int64_t>(pl.rows, N - i0);
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_contacts, dim3(grid), dim3(kBlock), pl.lds, e->stream, e->d_ip, (int)e->ip.size(), e->d_dp,
                       (int)e->dp.size(), e->d_ct_ip, e->d_ct_dp, P, W, dQ, N, i0, n, layout, pl.gx, pl.gm, e->m.ngeom,
                       dbits);
    HIP_TRY(hipGetLastError());
  }
  return MJPL_OK;
}

// One k_distance<mode> launch per kContactRows configurations: D [N][P] (DM_DIST), (C, pair) [N] (DM_CLEAR),
// (C, pair), grad [N][nplan], fromto [N][6], normal [N][3] and status [N] (DM_GRAD; fromto / normal may be null), or
// count [N] and K slots per configuration of pair, D (ddist), grad, fromto, normal and status (DM_NEAR: K = near_k,
// dcount; fromto / normal may be null), or gap and its pair (dclear, dpair) with slack and its pair (DM_SWEEP: dHD the
// travels beside dQ, dslack, dslack_pair; HD takes a second column set of the LDS carve).
int launch_distance(mjpl_engine *e, int mode, const double *dQ, int64_t N, int layout, double distmax, double *ddist,
                    double *dclear, int32_t *dpair, double *dgrad = nullptr, double *dfromto = nullptr,
                    double *dnormal = nullptr, int32_t *dstatus = nullptr, int near_k = 0, int32_t *dcount = nullptr,
                    const double *dHD = nullptr, double *dslack = nullptr, int32_t *dslack_pair = nullptr) {
  const int P = (int)e->ct_g1.size();
  if (N == 0 || (mode == DM_DIST && P == 0)) return MJPL_OK;
  const auto kernel = mode == DM_DIST    ? k_distance<DM_DIST>
                      : mode == DM_CLEAR ? k_distance<DM_CLEAR>
                      : mode == DM_GRAD  ? k_distance<DM_GRAD>
                      : mode == DM_NEAR  ? k_distance<DM_NEAR>
                                         : k_distance<DM_SWEEP>;
  PairLaunch pl;
  int rc = pair_query_prologue(e, kernel, N, &pl, mode == DM_SWEEP ? 2 : 1);
  if (rc != MJPL_OK) return rc;
  GradOut go = {};
  NearOut no = {};
  SweepIO sw = {};
  if (mode == DM_SWEEP) {
    sw.W = e->d_sweep_tab + 2 * e->qidx.size();
    sw.HD = dHD;
    sw.slack = dslack;
    sw.slack_pair = dslack_pair;
  }
  if (mode == DM_NEAR) {
    rc = e->d_nr_frames.reserve((size_t)pl.rows * e->qidx.size() * 6);
    if (rc != MJPL_OK) return rc;
    no.frames = e->d_nr_frames.p;
    no.K = near_k;
    no.count = dcount;
    no.pair = dpair;
    no.dist = ddist;
  }
  if (mode == DM_GRAD || mode == DM_NEAR) {
    const int nb = e->m.nbody, nplan = (int)e->qidx.size();
    rc = e->d_gr_scratch.reserve((size_t)pl.rows * nb * 7);
    if (rc != MJPL_OK) return rc;
    go.xpos = e->d_gr_scratch.p;
    go.xquat = e->d_gr_scratch.p + (size_t)pl.rows * nb * 3;
    go.nbody = nb;
    go.gcol = e->d_gr;
    go.gjnt = e->d_gr + (size_t)nplan * GC_LEN;
    go.gtin = go.gjnt + (size_t)e->m.njnt * JR_LEN;
    go.grad = dgrad;
    go.fromto = dfromto;
    go.normal = dnormal;
    go.status = dstatus;
  }
  for (int64_t i0 = 0; i0 < N; i0 += pl.rows) {
    const int64_t n = std::min<int64_t>(pl.rows, N - i0);
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    // (all outputs are indexed by the batch row i: whole arrays)
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), pl.lds, e->stream, e->d_ip, (int)e->ip.size(), e->d_dp,
                       (int)e->dp.size(), e->d_ct_ip, e->d_ct_dp, e->d_dt, P, dQ, N, i0, n, layout, distmax, pl.gx,
                       pl.gm, e->m.ngeom, ddist, dclear, dpair, go, no, sw);
    HIP_TRY(hipGetLastError());
  }
  return MJPL_OK;
}

int check_common(const mjpl_engine *e, const void *a, int64_t n, int layout) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  if (n < 0) return fail(MJPL_E_ARG, "negative batch size");
  if (n > 0 && !a) return fail(MJPL_E_ARG, "NULL batch pointer");
  if (layout != MJPL_SOA && layout != MJPL_AOS) return fail(MJPL_E_ARG, "layout must be MJPL_SOA or MJPL_AOS");
  return MJPL_OK;
}

// Argument checks of the pair queries: check_common, distmax > 0 (NaN refused; the contacts have none and pass +inf)
// and, when N > 0, every listed output non-null.
int check_query_args(const mjpl_engine *e, const void *Q, int64_t N, int layout, double distmax,
                     std::initializer_list<const void *> outs) {
  int rc = check_common(e, Q, N, layout);
  if (rc != MJPL_OK) return rc;
  if (!(distmax > 0)) return fail(MJPL_E_ARG, "distmax must be > 0 (NaN is refused), got %g", distmax);
  if (N > 0)
    for (const void *o : outs)
      if (!o) return fail(MJPL_E_ARG, "NULL output pointer");
  return MJPL_OK;
}

// ---- staging of the host-pointer entry points
// An array of a call in host memory: an input copied in, or an output copied back.  A null output is one the caller
// does not want: it gets no space and a null device pointer.  An output with `from` set is not written by the launch:
// it is copied from that device address after it (the edge pipeline's status word).  An output with `keep` set is one
// the launch writes only in part: the caller's bytes are copied in before it, so what it leaves alone comes back as it was.
struct HostIn {
  const void *host;
  size_t bytes;
};
struct HostOut {
  void *host;
  size_t bytes;
  const void *from = nullptr;
  bool keep = false;
};

constexpr size_t kSpanAlign = 256;  // every span starts at a multiple of this in its slot or in the pinned block
size_t span_bytes(size_t bytes) { return (bytes + kSpanAlign - 1) & ~(kSpanAlign - 1); }
// Calls whose spans total at most this go through the pinned block in one copy each way (small-batch tier 1)
constexpr size_t kPinnedCopyBytes = (size_t)256 << 10;

int pin_reserve(mjpl_engine *e, size_t bytes) {
  if (bytes <= e->h_pin_bytes) return MJPL_OK;
  if (e->h_pin) HIP_TRY(hipHostFree(e->h_pin));
  e->h_pin = nullptr;
  e->h_pin_bytes = 0;
  const size_t want = std::max<size_t>(bytes, 1 << 16);
  HIP_TRY(hipHostMalloc(&e->h_pin, want));
  e->h_pin_bytes = want;
  return MJPL_OK;
}

// The host-pointer form of an entry point: the inputs packed into the engine's input slot and the outputs into its
// output slot, launch(device inputs, device outputs) enqueued between the copies, the stream synchronised.  How the
// spans move goes by their total, wanted outputs or not (so the outputs a call asks for do not change its tier):
//   0. up to the option "zero_copy_bytes", if `small_tiers`: the kernels read the pinned block and write into it
//      themselves, over the bus -- no copy operation on the stream at all (a scalar valid_config pays launches and one
//      synchronisation);
//   1. up to kPinnedCopyBytes, if `small_tiers`: through the pinned block, one copy each way;
//   2. otherwise: one copy per span from and to the caller's pageable memory.
template <size_t NI, size_t NO, class F>
int staged(mjpl_engine *e, bool small_tiers, const HostIn (&in)[NI], const HostOut (&out)[NO], F launch) {
  HIP_TRY(hipSetDevice(e->device));
  size_t at_in[NI], at_out[NO], ib = 0, ob = 0, total = 0;
  for (size_t k = 0; k < NI; k++) {
    at_in[k] = ib;
    ib += span_bytes(in[k].bytes);
  }
  for (size_t k = 0; k < NO; k++) {
    at_out[k] = ob;
    total += span_bytes(out[k].bytes);
    if (out[k].host) ob += span_bytes(out[k].bytes);
  }
  total += ib;
  const int tier = !small_tiers ? 2 : total <= e->zero_copy_bytes ? 0 : total <= kPinnedCopyBytes ? 1 : 2;
  int rc;
  char *pin = nullptr, *dev_in, *dev_out;
  if (tier < 2) {
    if ((rc = pin_reserve(e, ib + ob)) != MJPL_OK) return rc;
    pin = (char *)e->h_pin;
    for (size_t k = 0; k < NI; k++) memcpy(pin + at_in[k], in[k].host, in[k].bytes);
    for (size_t k = 0; k < NO; k++)
      if (out[k].host && out[k].keep) memcpy(pin + ib + at_out[k], out[k].host, out[k].bytes);
  }
  if (tier == 0) {
    HIP_TRY(hipHostGetDevicePointer((void **)&dev_in, pin, 0));
    dev_out = dev_in + ib;
  } else {
    if ((rc = e->stage_in.reserve(ib, kStageFloor)) != MJPL_OK) return rc;
    if ((rc = e->stage_out.reserve(ob, kStageFloor)) != MJPL_OK) return rc;
    dev_in = e->stage_in.p;
    dev_out = e->stage_out.p;
    if (tier == 1) HIP_TRY(hipMemcpyAsync(dev_in, pin, ib, hipMemcpyHostToDevice, e->stream));
    for (size_t k = 0; k < NI && tier == 2; k++)
      if (in[k].bytes) HIP_TRY(hipMemcpyAsync(dev_in + at_in[k], in[k].host, in[k].bytes, hipMemcpyHostToDevice, e->stream));
    for (size_t k = 0; k < NO; k++) {
      const HostOut &o = out[k];
      if (!o.host || !o.keep || !o.bytes) continue;
      HIP_TRY(hipMemcpyAsync(dev_out + at_out[k], tier == 1 ? pin + ib + at_out[k] : (const char *)o.host, o.bytes,
                             hipMemcpyHostToDevice, e->stream));
    }
  }
  void *din[NI], *dout[NO];
  for (size_t k = 0; k < NI; k++) din[k] = dev_in + at_in[k];
  for (size_t k = 0; k < NO; k++) dout[k] = out[k].host ? dev_out + at_out[k] : nullptr;
  if ((rc = launch(din, dout)) != MJPL_OK) return rc;
  for (size_t k = 0; k < NO; k++) {
    const HostOut &o = out[k];
    if (!o.host || !o.bytes) continue;
    if (tier == 0 && o.from) HIP_TRY(hipMemcpyAsync(pin + ib + at_out[k], o.from, o.bytes, hipMemcpyDeviceToHost, e->stream));
    if (tier == 1 && o.from) HIP_TRY(hipMemcpyAsync(dout[k], o.from, o.bytes, hipMemcpyDeviceToDevice, e->stream));
    if (tier == 2) HIP_TRY(hipMemcpyAsync(o.host, o.from ? o.from : dout[k], o.bytes, hipMemcpyDeviceToHost, e->stream));
  }
  if (tier == 1) HIP_TRY(hipMemcpyAsync(pin + ib, dev_out, ob, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (size_t k = 0; k < NO && tier < 2; k++)
    if (out[k].host) memcpy(out[k].host, pin + ib + at_out[k], out[k].bytes);
  return MJPL_OK;
}

// The edge pipeline's status word (kStatus*: mjpl_filter.h, mjpl_fused.h) as a return code, with its message
int edge_status(int s) {
  if (s & (kStatusTailTimeout | kStatusFusedTimeout))
    return fail(MJPL_E_HIP, "a kernel of the edge pipeline gave up waiting (status %d: 2 = the tail kernel for its walking workgroups, 4 = a wave of the fused kernel for its work pool)", s);
  if (s & kStatusNonFinite) return fail(MJPL_E_NONFINITE, "an edge holds NaN/inf or needs more than %d waypoints", kMaxWaypoints);
  return MJPL_OK;
}

}  // namespace

// ------------------------------------------------------------------------------- C ABI

extern "C" {

const char *mjpl_last_error(void) { return g_err.c_str(); }

#ifdef MJPL_STAMPS
// diagnostic builds only: read and clear the phase counters of the queued interpreter
int mjpl_debug_stamps(unsigned long long *out) {
  unsigned long long z[16] = {0};
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mjpl::g_stamps), sizeof(z)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(mjpl::g_stamps), z, sizeof(z)) != hipSuccess) return -1;
  return 0;
}
#endif
const char *mjpl_version(void) { return "mjpl_hip 0.1 (gfx950)"; }

int mjpl_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

namespace {
// copy the model tables, the allowed body pairs and the environment overrides into a fresh engine
int engine_from_desc(mjpl_engine *e, const mjpl_model_desc *d, const int32_t *allowed_bodies, int32_t nallowed) {
  HostModel &m = e->m;
  m.nq = d->nq; m.njnt = d->njnt; m.nbody = d->nbody; m.ngeom = d->ngeom;
  m.body_parentid = copy_n(d->body_parentid, m.nbody);
  m.body_weldid = copy_n(d->body_weldid, m.nbody);
  m.body_jntadr = copy_n(d->body_jntadr, m.nbody);
  m.body_jntnum = copy_n(d->body_jntnum, m.nbody);
  m.body_pos = copy_n(d->body_pos, 3 * (size_t)m.nbody);
  m.body_quat = copy_n(d->body_quat, 4 * (size_t)m.nbody);
  m.jnt_type = copy_n(d->jnt_type, m.njnt);
  m.jnt_qposadr = copy_n(d->jnt_qposadr, m.njnt);
  m.jnt_axis = copy_n(d->jnt_axis, 3 * (size_t)m.njnt);
  m.jnt_pos = copy_n(d->jnt_pos, 3 * (size_t)m.njnt);
  m.qpos0 = copy_n(d->qpos0, m.nq);
  m.geom_type = copy_n(d->geom_type, m.ngeom);
  m.geom_bodyid = copy_n(d->geom_bodyid, m.ngeom);
  m.geom_contype = copy_n(d->geom_contype, m.ngeom);
  m.geom_conaffinity = copy_n(d->geom_conaffinity, m.ngeom);
  m.geom_size = copy_n(d->geom_size, 3 * (size_t)m.ngeom);
  m.geom_pos = copy_n(d->geom_pos, 3 * (size_t)m.ngeom);
  m.geom_quat = copy_n(d->geom_quat, 4 * (size_t)m.ngeom);
  m.geom_rbound = copy_n(d->geom_rbound, m.ngeom);
  m.geom_margin = copy_n(d->geom_margin, m.ngeom);
  for (int b = 0; b < m.nbody; b++)
    if (m.body_parentid[b] < 0 || m.body_parentid[b] > b || m.body_weldid[b] < 0 || m.body_weldid[b] > b)
      return (fail(MJPL_E_ARG, "body %d: parent/weld ids must precede the body", b));
  for (int g = 0; g < m.ngeom; g++)
    if (m.geom_bodyid[g] < 0 || m.geom_bodyid[g] >= m.nbody)
      return (fail(MJPL_E_ARG, "geom %d: body id out of range", g));
  for (int a = 0; a < nallowed; a++) {
    int b1 = allowed_bodies[2 * a], b2 = allowed_bodies[2 * a + 1];
    if (b1 < 0 || b2 < 0 || b1 >= m.nbody || b2 >= m.nbody)
      return (fail(MJPL_E_ARG, "allowed body pair %d out of range", a));
    e->allowed.insert({std::min(b1, b2), std::max(b1, b2)});
  }
  e->qidx.resize(m.nq);
  for (int k = 0; k < m.nq; k++) e->qidx[k] = k;
  e->qbase = m.qpos0;
  // (no switch is read from the environment here: mjpl_set_option; MJPL_DEBUG=1 lets the variables of old through, below)
  return MJPL_OK;
}
}  // namespace

void apply_debug_environment(mjpl_engine *e);

int mjpl_create(const mjpl_model_desc *d, const int32_t *allowed_bodies, int32_t nallowed,
                int32_t device, mjpl_engine **out) {
  if (!d || !out) return fail(MJPL_E_ARG, "mjpl_create: NULL argument");
  *out = nullptr;
  if (d->nq < 0 || d->njnt < 0 || d->nbody < 1 || d->ngeom < 0 || nallowed < 0)
    return fail(MJPL_E_ARG, "mjpl_create: negative size");
  if (d->nq != d->njnt) return fail(MJPL_E_JOINT, "nq != njnt: only 1-DoF joints are supported");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(MJPL_E_NODEVICE, "no HIP device available (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(MJPL_E_NODEVICE, "device %d out of range [0,%d)", device, ndev);

  mjpl_engine *e = new mjpl_engine();
  e->device = device;
  auto bail = [&](int rc) { mjpl_destroy(e); return rc; };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(MJPL_E_HIP, "hipSetDevice(%d) failed", device));
  if (hipGetDeviceProperties(&e->prop, device) != hipSuccess) return bail(fail(MJPL_E_HIP, "hipGetDeviceProperties failed"));
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) return bail(fail(MJPL_E_HIP, "hipStreamCreate failed"));
  if (hipMalloc(&e->d_status, sizeof(int)) != hipSuccess) return bail(fail(MJPL_E_HIP, "hipMalloc failed"));
  (void)hipMemset(e->d_status, 0, sizeof(int));

  int rc = engine_from_desc(e, d, allowed_bodies, nallowed);
  if (rc != MJPL_OK) return bail(rc);
  apply_debug_environment(e);
  if ((rc = compile_program(e)) != MJPL_OK || (rc = make_pair_tables(e)) != MJPL_OK || (rc = make_grad_table(e)) != MJPL_OK ||
      (rc = make_sweep_table(e, nullptr, nullptr)) != MJPL_OK)
    return bail(rc);
  *out = e;
  return MJPL_OK;
}

void mjpl_destroy(mjpl_engine *e) {
  if (e && e->d_fused_dbg.p && e->fused_dbg_path) {
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    std::vector<unsigned long long> h(kFusedDbgWaves * 8);
    if (hipMemcpy(h.data(), e->d_fused_dbg.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess)
      if (FILE *f = fopen(e->fused_dbg_path, "wb")) {
        fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
        fclose(f);
      }
  }
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->comm) (void)mjpl_comm_destroy(e);
  if (e->h_pin) (void)hipHostFree(e->h_pin);
  if (e->h_push_n) (void)hipHostFree(e->h_push_n);
  if (e->d_ip) (void)hipFree(e->d_ip);
  if (e->d_dp) (void)hipFree(e->d_dp);
  if (e->d_fp_base) (void)hipFree(e->d_fp_base);
  if (e->d_ucount_base) (void)hipFree(e->d_ucount_base);
  if (e->d_geomtab) (void)hipFree(e->d_geomtab);
  if (e->d_status) (void)hipFree(e->d_status);
  if (e->d_ct_ip) (void)hipFree(e->d_ct_ip);
  if (e->d_ct_dp) (void)hipFree(e->d_ct_dp);
  if (e->d_dt) (void)hipFree(e->d_dt);
  if (e->d_gr) (void)hipFree(e->d_gr);
  if (e->d_sweep_tab) (void)hipFree(e->d_sweep_tab);
  const hipStream_t stream = e->stream;
  delete e;  // (frees its DevBufs: with the device set, and before the stream goes)
  if (stream) (void)hipStreamDestroy(stream);
}

int mjpl_program_dump(const mjpl_model_desc *d, const int32_t *allowed_bodies, int32_t nallowed, const int32_t *qidx,
                      int32_t nplan, const double *qpos_base, double filter_tol, int32_t *ip, int32_t *nip, float *fp,
                      double *dp, int32_t *ntab, mjpl_program_info *info) {
  return mjpl_program_dump_pruned(d, allowed_bodies, nallowed, qidx, nplan, qpos_base, filter_tol, 1, ip, nip, fp, dp, ntab, info,
                                  nullptr, nullptr);
}

int mjpl_program_dump_pruned(const mjpl_model_desc *d, const int32_t *allowed_bodies, int32_t nallowed, const int32_t *qidx,
                             int32_t nplan, const double *qpos_base, double filter_tol, int32_t prune_pairs, int32_t *ip,
                             int32_t *nip, float *fp, double *dp, int32_t *ntab, mjpl_program_info *info, int32_t *dropped,
                             int32_t *ndropped) {
  if (!d || !nip || !ntab || !info) return fail(MJPL_E_ARG, "mjpl_program_dump: NULL argument");
  if (d->nq < 0 || d->njnt < 0 || d->nbody < 1 || d->ngeom < 0 || nallowed < 0) return fail(MJPL_E_ARG, "negative size");
  if (d->nq != d->njnt) return fail(MJPL_E_JOINT, "nq != njnt: only 1-DoF joints are supported");
  std::unique_ptr<mjpl_engine> e(new mjpl_engine());
  int rc = engine_from_desc(e.get(), d, allowed_bodies, nallowed);
  if (rc != MJPL_OK) return rc;
  if (qidx) {
    e->qidx.assign(qidx, qidx + nplan);
    for (int c : e->qidx)
      if (c < 0 || c >= d->nq) return fail(MJPL_E_ARG, "planning index %d out of range", c);
  }
  if (qpos_base) e->qbase.assign(qpos_base, qpos_base + d->nq);
  if (filter_tol > 0.0) { e->filter_tol_req = (float)filter_tol; e->filter_tol_user = true; }
  if (prune_pairs < 0 || prune_pairs > 2) return fail(MJPL_E_ARG, "mjpl_program_dump_pruned: prune_pairs must be 0, 1 or 2");
  e->prune_pairs = prune_pairs;
  if ((rc = compile_host(e.get())) != MJPL_OK) return rc;  // (host tables only: nothing is allocated or uploaded)
  if (ndropped) {  // (in: room for that many pairs in `dropped`; out: how many the program leaves out)
    const int32_t room = dropped ? *ndropped : 0;
    int32_t n = 0;
    for (const auto &gp : e->pruned) {
      if (n < room) { dropped[2 * n] = gp.first; dropped[2 * n + 1] = gp.second; }
      n++;
    }
    *ndropped = n;
  }
  memset(info, 0, sizeof(*info));
  info->hash = e->program_hash;
  // (maxs: the slot-file width of the FILTER kernels a library is built around -- 24 for the queued build of models with
  // moving boxes; immediate: only the immediate interpreter serves this program, nothing to specialise)
  info->maxs = e->filter_mbox() ? kQueuedMaxSlots : e->lay.maxs; info->wbox = e->lay.wbox; info->mbox = e->lay.mbox || e->filter_mbox();
  info->immediate = e->immediate() || (e->exact_general() && !e->filter_mbox());
  info->filter_usable = e->fb.usable; info->filter_tol = e->fb.tol; info->nslots = e->lay.nslots; info->nsave = e->lay.nsave;
  info->spec_abi = MJPL_SPEC_ABI;
  info->robot_hash = e->robot_hash;
  info->scene_rows = kSceneRows;
  info->scene_ok = e->scene.empty() ? 0 : 1;
  const int32_t want_ip = (int32_t)e->ip.size(), want_tab = (int32_t)e->fp.size();
  const bool fits = ip && fp && *nip >= want_ip && *ntab >= want_tab;
  *nip = want_ip;
  *ntab = want_tab;
  if (!ip && !fp && !dp) return MJPL_OK;  // size query
  if (!fits) return fail(MJPL_E_CAPACITY, "mjpl_program_dump: buffers too small (%d control words, %d constants)", want_ip, want_tab);
  memcpy(ip, e->ip.data(), e->ip.size() * sizeof(int));
  memcpy(fp, e->fp.data(), e->fp.size() * sizeof(float));
  if (dp) memcpy(dp, e->dp.data(), e->dp.size() * sizeof(double));
  return MJPL_OK;
}

int mjpl_program_dump_never_touch(const mjpl_model_desc *d, const int32_t *allowed_bodies, int32_t nallowed, const int32_t *qidx,
                                  int32_t nplan, const double *qpos_base, double filter_tol, int32_t prune_pairs,
                                  int32_t prune_contacts, int32_t *pairs, int32_t *npairs, int32_t *evals, uint64_t *hash,
                                  uint64_t *tables_hash) {
  if (!d || !npairs) return fail(MJPL_E_ARG, "mjpl_program_dump_never_touch: NULL argument");
  if (d->nq < 0 || d->njnt < 0 || d->nbody < 1 || d->ngeom < 0 || nallowed < 0) return fail(MJPL_E_ARG, "negative size");
  if (d->nq != d->njnt) return fail(MJPL_E_JOINT, "nq != njnt: only 1-DoF joints are supported");
  if (prune_pairs < 0 || prune_pairs > 2 || prune_contacts < 0 || prune_contacts > (1 << 24))
    return fail(MJPL_E_ARG, "mjpl_program_dump_never_touch: prune_pairs must be 0, 1 or 2, prune_contacts 0 .. 2^24");
  std::unique_ptr<mjpl_engine> e(new mjpl_engine());
  int rc = engine_from_desc(e.get(), d, allowed_bodies, nallowed);
  if (rc != MJPL_OK) return rc;
  if (qidx) {
    e->qidx.assign(qidx, qidx + nplan);
    for (int c : e->qidx)
      if (c < 0 || c >= d->nq) return fail(MJPL_E_ARG, "planning index %d out of range", c);
  }
  if (qpos_base) e->qbase.assign(qpos_base, qpos_base + d->nq);
  if (filter_tol > 0.0) { e->filter_tol_req = (float)filter_tol; e->filter_tol_user = true; }
  e->prune_pairs = prune_pairs;
  e->prune_contacts = prune_contacts;
  if ((rc = compile_host(e.get())) != MJPL_OK) return rc;
  const int32_t room = pairs ? *npairs : 0;  // (in: room for that many pairs; out: how many there are)
  int32_t n = 0;
  for (const auto &gp : e->never_touch) {
    if (n < room) { pairs[2 * n] = gp.first; pairs[2 * n + 1] = gp.second; }
    n++;
  }
  *npairs = n;
  if (evals) *evals = e->never_valid ? e->prune_contact_evals : 0;
  if (hash) *hash = e->program_hash;
  if (tables_hash) *tables_hash = hash_program(e->lay, e->ip, e->fp, e->dp, GeomPairs());
  return MJPL_OK;
}

int mjpl_sweep_levers(const mjpl_model_desc *d, const int32_t *allowed_bodies, int32_t nallowed, const int32_t *qidx,
                      int32_t nplan, const double *qpos_base, const double *lo, const double *hi, double *W, int64_t cap) {
  if (!d) return fail(MJPL_E_ARG, "mjpl_sweep_levers: NULL argument");
  if (d->nq < 0 || d->njnt < 0 || d->nbody < 1 || d->ngeom < 0 || nallowed < 0) return fail(MJPL_E_ARG, "negative size");
  if (d->nq != d->njnt) return fail(MJPL_E_JOINT, "nq != njnt: only 1-DoF joints are supported");
  std::unique_ptr<mjpl_engine> e(new mjpl_engine());
  int rc = engine_from_desc(e.get(), d, allowed_bodies, nallowed);
  if (rc != MJPL_OK) return rc;
  if (qidx) {
    e->qidx.assign(qidx, qidx + nplan);
    for (int c : e->qidx)
      if (c < 0 || c >= d->nq) return fail(MJPL_E_ARG, "planning index %d out of range", c);
  }
  if (qpos_base) e->qbase.assign(qpos_base, qpos_base + d->nq);
  for (size_t k = 0; k < e->qidx.size(); k++) {
    const double l = lo ? lo[k] : -INFINITY, h = hi ? hi[k] : INFINITY;
    if (!(l <= h)) return fail(MJPL_E_ARG, "bounds of planning column %d: lo %g, hi %g (NaN and lo > hi are refused)", (int)k, l, h);
  }
  if ((rc = compile_host(e.get())) != MJPL_OK) return rc;  // (host tables only: nothing is allocated or uploaded)
  std::vector<int> cip;
  std::vector<double> cdp;
  build_contact_table(e.get(), cip, cdp);
  const std::vector<double> t = build_sweep_table(e.get(), lo, hi);
  const int64_t P = (int64_t)e->ct_g1.size();
  if (W && cap >= (int64_t)t.size()) memcpy(W, t.data(), t.size() * sizeof(double));
  else if (W) return fail(MJPL_E_CAPACITY, "mjpl_sweep_levers: room for %lld doubles, the table has %zu", (long long)cap, t.size());
  return (int)P;
}

int mjpl_spec_probe(uint64_t hash, int32_t generic) {
  return find_spec(hash, generic != 0) ? 1 : 0;
}

int mjpl_spec_loaded(const mjpl_engine *e) { return (e && e->spec) ? (e->spec_generic ? 2 : 1) : 0; }

int mjpl_set_spec(mjpl_engine *e, int32_t enable) {
  if (!e) return fail(MJPL_E_ARG, "mjpl_set_spec: NULL engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->spec_off = enable == 0;
  e->spec_generic_only = enable == 2;
  return compile_program(e);  // (a scene-generic library wants its cull table in front of the float32 tables)
}

int mjpl_set_planning(mjpl_engine *e, const int32_t *qidx, int32_t nplan, const double *qpos_base) {
  if (!e || nplan < 0 || (nplan > 0 && !qidx)) return fail(MJPL_E_ARG, "mjpl_set_planning: bad argument");
  std::vector<int> q(qidx, qidx + nplan);
  std::vector<char> seen(e->m.nq, 0);
  for (int c : q) {
    if (c < 0 || c >= e->m.nq || seen[c]) return fail(MJPL_E_ARG, "planning index %d invalid or repeated", c);
    seen[c] = 1;
  }
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->qidx = q;
  if (qpos_base) e->qbase.assign(qpos_base, qpos_base + e->m.nq);
  const int rc = compile_program(e);
  if (rc != MJPL_OK) return rc;
  MJPL_TRY(make_grad_table(e));
  return make_sweep_table(e, nullptr, nullptr);
}

int mjpl_set_filter(mjpl_engine *e, int32_t enable, double tol) {
  if (!e) return fail(MJPL_E_ARG, "mjpl_set_filter: NULL engine");
  if (enable && !(tol > 0.0 && tol < 1.0)) return fail(MJPL_E_ARG, "filter tolerance must be in (0, 1) metres");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->filter = enable != 0;
  if (enable && (!e->filter_tol_user || (float)tol != e->filter_tol_req)) {
    e->filter_tol_req = (float)tol;
    e->filter_tol_user = true;
    return compile_program(e);
  }
  return MJPL_OK;
}

int64_t mjpl_filter_last_undecided(mjpl_engine *e) {
  if (!e || !e->filter || !e->fb.usable || !e->d_ucount) return 0;
  int n[5 * kCtr];
  if (hipSetDevice(e->device) != hipSuccess) return -1;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return -1;
  if (hipMemcpy(n, e->d_ucount, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return (int64_t)n[0] + n[kCtr];
}

// Diagnostic: the (edge, check index, geom a, geom b) records the last filter launch handed to the exact pair
// kernel -- which pairs the float32 filter could not decide.  Returns how many there were (the arrays receive up to
// `cap` of them), or -1.
int64_t mjpl_filter_undecided_pairs(mjpl_engine *e, int32_t *edge, int32_t *idx, int32_t *ga, int32_t *gb, int64_t cap) {
  if (!e || !e->filter || !e->fb.usable || !e->d_ucount || !e->d_ucedge.p) return 0;
  if (hipSetDevice(e->device) != hipSuccess) return -1;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return -1;
  int n = 0;
  if (hipMemcpy(&n, e->d_ucount + kCtr, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const size_t m = (size_t)std::max<int64_t>(0, std::min<int64_t>(std::min<int64_t>(n, cap), (int64_t)e->uc_cap));
  int32_t *dst[4] = {edge, idx, ga, gb};
  const int *src[4] = {e->d_ucedge.p, e->d_ucidx.p, e->d_ucga.p, e->d_ucgb.p};
  for (int k = 0; k < 4; k++)
    if (dst[k] && m && hipMemcpy(dst[k], src[k], m * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}

namespace {
// the launch's counters on the host (synchronises the stream)
bool read_counters(mjpl_engine *e, std::vector<int> &n) {
  n.assign((size_t)kNumCtr * kCtr, 0);
  if (hipSetDevice(e->device) != hipSuccess) return false;
  if (hipStreamSynchronize(e->stream) != hipSuccess) return false;
  return hipMemcpy(n.data(), e->d_ucount, n.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
}
}  // namespace

int64_t mjpl_filter_last_interior_edges(mjpl_engine *e) {
  if (!e || !e->filter || !e->d_ucount) return -1;
  std::vector<int> n;
  if (!read_counters(e, n)) return -1;
  int64_t total = n[2 * kCtr];  // (one counter without the lane-per-waypoint pass, one per region with it)
  for (int r = 0; r < kItemRegions; r++) total += n[(size_t)(5 + kItemRegions + r) * kCtr];
  return total;
}

int64_t mjpl_filter_last_items(mjpl_engine *e) {
  if (!e || !e->filter || !e->d_ucount) return -1;
  std::vector<int> n;
  if (!read_counters(e, n)) return -1;
  int64_t total = 0;  // (reserved slots, as before: a region's surplus went to the walking kernel)
  for (int r = 0; r < kItemRegions; r++) total += n[(size_t)(5 + r) * kCtr];
  return total;
}

int64_t mjpl_filter_last_certified(mjpl_engine *e) {
  if (!e || !e->filter || !e->d_ucount) return -1;
  std::vector<int> n;
  if (!read_counters(e, n)) return -1;
  return n[(size_t)kCtrCertified * kCtr];
}

int mjpl_get_info(const mjpl_engine *e, mjpl_info *out) {
  if (!e || !out) return fail(MJPL_E_ARG, "mjpl_get_info: NULL argument");
  memset(out, 0, sizeof(*out));
  out->device = e->device;
  out->nplan = (int)e->qidx.size();
  out->nmoving_geoms = e->lay.nmoving;
  out->nstatic_geoms = e->lay.nworld();
  out->npairs = e->lay.npairs;
  out->npairs_world = e->lay.npairs_world;
  out->nslots = e->lay.nslots;
  out->nsaves = e->lay.nsave;
  out->lds_bytes_configs = (int)lds_bytes(e, 1);
  out->lds_bytes_edges = (int)lds_bytes(e, 1);
  out->filter_enabled = (e->filter && e->fb.usable) ? 1 : 0;
  out->filter_tol = e->fb.tol;
  out->filter_max_coord = (float)e->fb.fmax_coord;
  out->filter_err_a = (float)e->fb.ferr_a;
  out->filter_err_b = (float)e->fb.ferr_b;
  out->filter_poisoned_geoms = e->fb.npoisoned;
  out->filter_interpreter = e->immediate() ? 2 : (e->filter_mbox() ? 1 : 0);
  out->filter_block_threads = e->immediate() ? kBlock : kFilterBlock;
  out->lds_bytes_filter = (int)lds_bytes(e, 1, sizeof(float), out->filter_block_threads, !e->immediate(),
                                         e->immediate() ? sizeof(double) : sizeof(float));
  // what an ordinary edge launch would do (an empty batch: below every threshold of the batch size, so the library
  // is the program's own)
  const EdgePlan p = plan_edges(e, 0, 0, false);
  out->persistent_kernels = p.persistent ? 1 : 0;
  out->fused_tail = p.tail ? 1 : 0;
  out->fused_edges = (p.pipe == EdgePipe::kFused || p.pipe == EdgePipe::kF64Pool) ? 1 : 0;  // (filter off: the float64 checks through the pool)
  out->fused_waves = p.fwaves;
  out->block_threads = kBlock;
  out->compute_units = e->prop.multiProcessorCount;
  strncpy(out->arch, e->prop.gcnArchName, sizeof(out->arch) - 1);
  return MJPL_OK;
}

// ---- device-resident

int mjpl_check_configs_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, uint8_t *dvalid) {
  int rc = check_common(e, dQ, N, layout);
  if (rc != MJPL_OK) return rc;
  if (N > 0 && !dvalid) return fail(MJPL_E_ARG, "NULL output pointer");
  HIP_TRY(hipSetDevice(e->device));
  return launch_configs(e, dQ, N, layout, dvalid, nullptr);
}

int mjpl_check_configs_bits_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, uint64_t *dbits) {
  int rc = check_common(e, dQ, N, layout);
  if (rc != MJPL_OK) return rc;
  if (N > 0 && !dbits) return fail(MJPL_E_ARG, "NULL output pointer");
  HIP_TRY(hipSetDevice(e->device));
  return launch_configs(e, dQ, N, layout, nullptr, reinterpret_cast<unsigned long long *>(dbits));
}

int mjpl_check_edges_dev(mjpl_engine *e, const double *dQA, const double *dQB, int64_t E, double step_dist,
                         int32_t layout, int32_t flags, uint8_t *dvalid, int32_t *dfirst_bad) {
  int rc = check_common(e, dQA, E, layout);
  if (rc != MJPL_OK) return rc;
  if (E > 0 && (!dQB || !dvalid)) return fail(MJPL_E_ARG, "NULL pointer");
  if (!(step_dist > 0.0)) return fail(MJPL_E_ARG, "`step_dist` must be > 0");
  HIP_TRY(hipSetDevice(e->device));
  return launch_edges(e, dQA, dQB, E, step_dist, layout, flags, dvalid, dfirst_bad, false);
}

int mjpl_take_status(mjpl_engine *e, int32_t *status) {
  if (!e || !status) return fail(MJPL_E_ARG, "mjpl_take_status: NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  int s = 0;
  HIP_TRY(hipMemcpyAsync(&s, e->d_status, sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  const int rc = edge_status(s);
  if (rc == MJPL_E_HIP) return rc;
  *status = rc;
  return MJPL_OK;
}

// ---- options through the ABI (include/mjpl_hip.h).  One table: name -> how to read it, how to set it.
namespace {
double kt_sum(mjpl_engine *e, int c) {
  if (hipDeviceSynchronize() != hipSuccess) return -1.0;
  double sum = 0;
  for (int k = 0; k + 1 < e->kt_used[c]; k += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, e->kt_ev[c][(size_t)k], e->kt_ev[c][(size_t)k + 1]) != hipSuccess) return -1.0;
    sum += ms;
  }
  return sum;
}
// (what the last look-up on the engine's scratch left at byte `at` of its arena; false: no such bytes, or the copy failed)
bool nn_arena_read(mjpl_engine *e, size_t at, void *dst, size_t bytes) {
  if (at + bytes > e->nn.arena.cap) return false;
  return hipStreamSynchronize(e->stream) == hipSuccess && hipMemcpy(dst, e->nn.arena.p + at, bytes, hipMemcpyDeviceToHost) == hipSuccess;
}
struct EngineOption {
  const char *name;
  double (*get)(mjpl_engine *);
  bool (*set)(mjpl_engine *, double);  // false: value out of range
};
#define MJPL_OPT_BOOL(NAME, FIELD) \
  {NAME, [](mjpl_engine *e) { return (double)(e->FIELD ? 1 : 0); }, [](mjpl_engine *e, double v) { e->FIELD = v != 0.0; return true; }}
#define MJPL_OPT_INT(NAME, FIELD, LO, HI)                                   \
  {NAME, [](mjpl_engine *e) { return (double)e->FIELD; }, [](mjpl_engine *e, double v) { \
     if (!(v >= (double)(LO) && v <= (double)(HI))) return false;            \
     e->FIELD = (decltype(e->FIELD))v;                                       \
     return true;                                                            \
   }}
const EngineOption kEngineOptions[] = {
    // ---- what shapes the compiled model or the launch pipeline (take effect at the next mjpl_set_planning / mjpl_set_spec /
    //      mjpl_set_filter, which compile again; the launch-time ones at the next launch)
    MJPL_OPT_BOOL("filter", filter),
    MJPL_OPT_INT("prune_pairs", prune_pairs, 0, 2),
    {"pairs_pruned", [](mjpl_engine *e) { return (double)e->lay.npruned; }, nullptr},
    {"prune_evals", [](mjpl_engine *e) { return (double)(e->prune_pairs ? e->prune_evals : 0); }, nullptr},
    MJPL_OPT_INT("prune_contacts", prune_contacts, 0, 1 << 24),
    {"pairs_never_touch", [](mjpl_engine *e) { return (double)e->never_touch.size(); }, nullptr},
    {"prune_contact_evals", [](mjpl_engine *e) { return (double)(e->never_valid ? e->prune_contact_evals : 0); }, nullptr},
    MJPL_OPT_BOOL("two_pass", two_pass),
    MJPL_OPT_BOOL("force_immediate", force_immediate),
    MJPL_OPT_BOOL("expand", expand),
    MJPL_OPT_BOOL("persist", persist),
    MJPL_OPT_BOOL("tail", fused_tail),
    MJPL_OPT_BOOL("fused", fused),
    MJPL_OPT_INT("fused_policy", fused_policy, -1000000, 1000000),
    MJPL_OPT_BOOL("fused_cert", fused_cert),
    MJPL_OPT_INT("fused_cert_min_edges", fused_cert_min_edges, 0, 1ll << 40),
    {"spec_cert_loaded", [](mjpl_engine *e) { return (double)(e->spec_cert ? 1 : 0); }, nullptr},
    MJPL_OPT_BOOL("f64_spec", f64_spec),
    MJPL_OPT_INT("fused_pool", fused_pool_cap, 0, 1 << 30),
    MJPL_OPT_BOOL("fused_mbox", fused_mbox),
    MJPL_OPT_BOOL("f64_queued", f64_queued),
    MJPL_OPT_INT("fused_single", fused_single_max, 0, 1 << 30),
    MJPL_OPT_INT("fused_kmax", fused_kmax, 2, 1 << 16),
    MJPL_OPT_INT("item_cap", item_cap_limit, 64, 1ll << 40),
    MJPL_OPT_INT("uc_cap", uc_cap_limit, 1, 1ll << 40),
    {"filter_tol", [](mjpl_engine *e) { return (double)e->filter_tol_req; },
     [](mjpl_engine *e, double v) { if (!(v > 0.0 && v < 1.0)) return false; e->filter_tol_req = (float)v; e->filter_tol_user = true; return true; }},
    MJPL_OPT_INT("zero_copy_bytes", zero_copy_bytes, 0, 1ll << 40),
    // ---- projection / IK rows
    MJPL_OPT_INT("rows_g", rows_g, 0, 64),
    MJPL_OPT_BOOL("pose_spec", pose_spec),
    MJPL_OPT_INT("pose_phase_steps", pose_phase_steps, 0, 1 << 20),
    // ---- the planner (read by mjpl_rrt_create)
    MJPL_OPT_INT("rrt_trace", rrt_trace, 0, 2),
    MJPL_OPT_BOOL("rrt_early_nn", rrt.early_nn),
    MJPL_OPT_INT("rrt_early_lanes", rrt.early_lanes, 1, 1 << 30),
    MJPL_OPT_INT("rrt_early_min_nodes", rrt.early_min_nodes, 1, 1ll << 40),
    MJPL_OPT_BOOL("rrt_early_next", rrt.early_next),
    MJPL_OPT_INT("rrt_proj_steps", rrt.proj_steps, 1, 1 << 30),
    MJPL_OPT_INT("rrt_proj_slots", rrt.proj_slots, 1, 1ll << 40),
    {"rrt_proj_g", [](mjpl_engine *e) { return (double)e->rrt.proj_g; },
     [](mjpl_engine *e, double v) { const int g = (int)v; e->rrt.proj_g = (g == 1 || g == 4 || g == 8 || g == 16 || g == 64) ? g : 0; return true; }},
    MJPL_OPT_BOOL("rrt_ahead", rrt.ahead),
    MJPL_OPT_INT("rrt_ahead_lanes", rrt.ahead_lanes, 1, 1 << 30),
    MJPL_OPT_INT("rrt_proj_waves", rrt.proj_waves, 1, 1 << 20),
    // ---- nearest neighbour
    MJPL_OPT_BOOL("nn_cells", nn_cells),
    MJPL_OPT_BOOL("nn_home", nn_home),
    MJPL_OPT_BOOL("nn_second_screen", nn_second_screen),
    MJPL_OPT_BOOL("nn_mfma", nn_mfma),
    {"nn_cells_min_nodes", [](mjpl_engine *e) { return (double)e->nn_cells_min; },
     [](mjpl_engine *e, double v) { if (!(v >= 0 && v < 9e15)) return false; e->nn_cells_min = (int64_t)v; return true; }},
    {"nn_cells_sample", [](mjpl_engine *e) { return (double)e->nn_cells_sample; },
     [](mjpl_engine *e, double v) { if (!(v >= 32 && v < 9e15)) return false; e->nn_cells_sample = std::max<int64_t>(1024, (int64_t)v) / 32 * 32; return true; }},
    {"nn_sample", [](mjpl_engine *e) { return (double)e->nn_sample; },
     [](mjpl_engine *e, double v) { if (!(v >= 32 && v < 9e15)) return false; e->nn_sample = std::max<int64_t>(1024, (int64_t)v) / 32 * 32; return true; }},
    // (read-only, like the two below and mjpl_nearest_last_screen: the last look-up on the engine's own scratch -- none of the
    //  planner's on its second stream -- took the cell-ordered scan)
    {"nn_last_cells", [](mjpl_engine *e) { return e->nn.last.cells ? 1.0 : 0.0; }, nullptr},
    // ---- trajectories (launch_topp_profile; read at the next call: more or fewer launches, the same bits)
    MJPL_OPT_INT("topp_chunk_bytes", topp_chunk_bytes, 1, 1ll << 40),
    {"topp_last_chunks", [](mjpl_engine *e) { return (double)e->topp_last_chunks; }, nullptr},
    // ---- path shortcutting (launch_shortcut; the chunk size is read at the next call: more or fewer launches, the same bits)
    MJPL_OPT_INT("shortcut_chunk_bytes", shortcut_chunk_bytes, 1, 1ll << 40),
    {"shortcut_last_chunks", [](mjpl_engine *e) { return (double)e->shortcut_last_chunks; }, nullptr},
    {"shortcut_last_rounds", [](mjpl_engine *e) { return (double)e->shortcut_last_rounds; }, nullptr},
    {"shortcut_last_edges", [](mjpl_engine *e) { return (double)e->shortcut_last_edges; }, nullptr},
    {"shortcut_last_propose_ms", [](mjpl_engine *e) { return e->shortcut_last_ms[0]; }, nullptr},
    {"shortcut_last_validate_ms", [](mjpl_engine *e) { return e->shortcut_last_ms[1]; }, nullptr},
    {"shortcut_last_commit_ms", [](mjpl_engine *e) { return e->shortcut_last_ms[2]; }, nullptr},
    // ---- planning in lockstep (launch_plan; the chunk size is read at the next call: more or fewer launches, the same bits)
    MJPL_OPT_INT("plan_chunk_bytes", plan_chunk_bytes, 1, 1ll << 40),
    {"plan_last_chunks", [](mjpl_engine *e) { return (double)e->plan_last_chunks; }, nullptr},
    {"plan_last_rounds", [](mjpl_engine *e) { return (double)e->plan_last_rounds; }, nullptr},
    {"plan_last_edges", [](mjpl_engine *e) { return (double)e->plan_last_edges; }, nullptr},
    {"plan_last_propose_ms", [](mjpl_engine *e) { return e->plan_last_ms[0]; }, nullptr},
    {"plan_last_validate_ms", [](mjpl_engine *e) { return e->plan_last_ms[1]; }, nullptr},
    {"plan_last_commit_ms", [](mjpl_engine *e) { return e->plan_last_ms[2]; }, nullptr},
    {"plan_last_project_ms", [](mjpl_engine *e) { return e->plan_last_ms[3]; }, nullptr},
    // ---- roadmap planning (launch_roadmap_build, launch_roadmap_query; read at the next call: more or fewer launches, the same bits)
    MJPL_OPT_INT("roadmap_chunk_bytes", roadmap_chunk_bytes, 1, 1ll << 40),
    MJPL_OPT_INT("roadmap_lds_nodes", roadmap_lds_nodes, 0, kRoadmapLdsNodes),
    {"roadmap_last_edges", [](mjpl_engine *e) { return (double)e->roadmap_last_edges; }, nullptr},
    {"roadmap_last_chunks", [](mjpl_engine *e) { return (double)e->roadmap_last_chunks; }, nullptr},
    {"roadmap_last_sweeps", [](mjpl_engine *e) { return (double)e->roadmap_last_sweeps; }, nullptr},
    {"roadmap_last_phase0_ms", [](mjpl_engine *e) { return e->roadmap_last_ms[0]; }, nullptr},
    {"roadmap_last_phase1_ms", [](mjpl_engine *e) { return e->roadmap_last_ms[1]; }, nullptr},
    {"roadmap_last_phase2_ms", [](mjpl_engine *e) { return e->roadmap_last_ms[2]; }, nullptr},
    {"roadmap_last_phase3_ms", [](mjpl_engine *e) { return e->roadmap_last_ms[3]; }, nullptr},
    {"kernel_timer", [](mjpl_engine *e) { return (double)e->kt_mode; },
     [](mjpl_engine *e, double v) {
       if (!(v >= 0 && v <= 3)) return false;
       e->kt_mode = (int)v;
       e->kt_used[0] = e->kt_used[1] = 0;
       for (int c = 0; c < 2; c++)  // (the events of a run's first launches are made here, not inside what is being timed)
         while (((int)v >> c & 1) && e->kt_ev[c].size() < 1024) {
           hipEvent_t ev = nullptr;
           if (hipEventCreate(&ev) != hipSuccess) break;
           e->kt_ev[c].push_back(ev);
         }
       return true;
     }},
    {"kernel_timer_launches", [](mjpl_engine *e) { return (double)(e->kt_used[0] / 2); }, nullptr},
    {"kernel_timer2_launches", [](mjpl_engine *e) { return (double)(e->kt_used[1] / 2); }, nullptr},
    // (read-only; synchronise the device: the launches may be on the planner's second stream)
    {"kernel_timer_ms", [](mjpl_engine *e) { return kt_sum(e, 0); }, nullptr},
    {"kernel_timer2_ms", [](mjpl_engine *e) { return kt_sum(e, 1); }, nullptr},
    // (2: the cell-ordered scan counts the pairs that reach their exact evaluation -- "nn_last_exact_pairs"; answers unchanged.
    //  A switch that dropped them unevaluated, for timing, gave wrong answers by design and is not in the product: see round 5.)
    {"nn_probe", [](mjpl_engine *e) { return (double)e->nn_probe; },
     [](mjpl_engine *e, double v) { if (v != 0.0 && v != 2.0) return false; e->nn_probe = (int)v; return true; }},
    {"nn_last_exact_pairs",  // (read-only; synchronises; counted only with "nn_probe" = 2, by a cell-ordered scan: else -1)
     [](mjpl_engine *e) {
       unsigned x[4] = {0, 0, 0, 0};
       if (!e->nn.last.cells || !nn_arena_read(e, 0, x, sizeof(x))) return -1.0;
       return (double)x[3];
     },
     nullptr},
    // (read-only; synchronises: the share of the tree's sub-chunks a wave of the last cell-ordered scan had on its list, averaged)
    {"nn_last_candidate_fraction",
     [](mjpl_engine *e) {
       const NnScratch::Last &last = e->nn.last;
       if (!last.cells || last.waves < 1 || last.nsub < 1) return -1.0;
       std::vector<int32_t> c((size_t)last.waves);
       if (!nn_arena_read(e, last.count_at, c.data(), c.size() * sizeof(int32_t))) return -1.0;
       double sum = 0;
       for (int32_t v : c) sum += v;
       return sum / ((double)c.size() * last.nsub);
     },
     nullptr},
};
#undef MJPL_OPT_INT
#undef MJPL_OPT_BOOL
}  // namespace

int mjpl_set_option(mjpl_engine *e, const char *name, double value) {
  if (!e || !name) return fail(MJPL_E_ARG, "mjpl_set_option: NULL argument");
  for (const EngineOption &o : kEngineOptions)
    if (strcmp(o.name, name) == 0) {
      if (!o.set) return fail(MJPL_E_ARG, "mjpl_set_option: \"%s\" is read-only", name);
      if (!(value == value) || !o.set(e, value)) return fail(MJPL_E_ARG, "mjpl_set_option: value %g out of range for \"%s\"", value, name);
      return MJPL_OK;
    }
  return fail(MJPL_E_ARG, "mjpl_set_option: unknown option \"%s\"", name);
}

// MJPL_DEBUG=1 (and only then): every writable option NAME is also taken from the variable MJPL_<NAME> when an engine is
// made -- for shell tools and A/B scripts (tools/README.md).  The library reads no other switch from the environment.
void apply_debug_environment(mjpl_engine *e) {
  const char *dbg = getenv("MJPL_DEBUG");
  if (!dbg || atoi(dbg) == 0) return;
  for (const EngineOption &o : kEngineOptions) {
    if (!o.set) continue;
    std::string var = "MJPL_";
    for (const char *c = o.name; *c; c++) var += (char)toupper((unsigned char)*c);
    if (const char *v = getenv(var.c_str())) (void)o.set(e, atof(v));
  }
  e->fused_dbg_path = getenv("MJPL_FUSED_DEBUG");  // (a file the fused kernel's per-wave accounting is written to: tools/fused_debug.py)
}

int32_t mjpl_option_count(void) { return (int32_t)(sizeof(kEngineOptions) / sizeof(kEngineOptions[0])); }

const char *mjpl_option_name(int32_t index, int32_t *writable) {
  if (index < 0 || index >= mjpl_option_count()) return nullptr;
  if (writable) *writable = kEngineOptions[index].set ? 1 : 0;
  return kEngineOptions[index].name;
}

int mjpl_set_spec_dir(const char *dir) {
  std::lock_guard<std::mutex> lock(spec_mutex());
  spec_dir_store() = dir ? dir : "";
  return MJPL_OK;
}

int mjpl_get_option(mjpl_engine *e, const char *name, double *value) {
  if (!e || !name || !value) return fail(MJPL_E_ARG, "mjpl_get_option: NULL argument");
  for (const EngineOption &o : kEngineOptions)
    if (strcmp(o.name, name) == 0) { *value = o.get(e); return MJPL_OK; }
  return fail(MJPL_E_ARG, "mjpl_get_option: unknown option \"%s\"", name);
}

int32_t mjpl_nearest_last_screen(mjpl_engine *e) {
  if (!e) return -1;
  if (e->nn.last.path != 2) return e->nn.last.path;
  unsigned x[2] = {0, 0};
  if (hipSetDevice(e->device) != hipSuccess || !nn_arena_read(e, 0, x, sizeof(x))) return -1;
  return x[1] ? 1 : 2;  // (coordinates too large for binary16: the binary32 screen ran)
}

}  // extern "C"

// ---- nearest neighbour (mjpl_nearest.h, mjpl_nearest_cells.h): a plan, a scratch (NnScratch), a function per stage

// ---- What one look-up will do, decided before anything is reserved or enqueued (no HIP call in here).
//   kLds       more planning columns than the chunked kernels take (or no nodes): k_nearest, a tile of nodes in LDS
//   kPlain     the float64 scan: 512 queries per block x node chunks, then a reduction over the chunks
//   kScreen32  large trees and query sets.  First a strided sample of the nodes, exactly: every query gets a bound close to
//              its answer.  Then the binary32-screened scan of all nodes, eight queries per lane, which evaluates exactly
//              only what lies within that bound
//   kMfma      ... the screened scan on the matrix cores (nplan <= 7), unless some coordinate is too large for binary16 --
//              which the device finds out while it packs the operands: then those kernels return at once and the float64
//              sample scan and the binary32 screen run (which in turn return at once when the matrix cores serve the call)
//   kCells     ... the cell-ordered scan (mjpl_nearest_cells.h): nodes sorted along a space-filling curve, queries by where
//              on it their bound was found, a wave scans the sub-chunks some query of it can have its answer in
enum class NnPath { kLds, kPlain, kScreen32, kMfma, kCells };

struct NnPlan {
  NnPath path;
  int nplan;
  unsigned rgridM;  // one thread per query, kBlock of them
  // float64 scan: blocks of queries, node chunks of `chunk`, partial rows the scratch holds
  int64_t qtiles, nchunks, chunk;
  size_t maxchunks;
  // the float64 scan of the sample: every stride-th node, nsamp64 of them in chunks of ch0 (nc0 planned, nch0 launched)
  int64_t stride, nc0, ch0, nsamp64, nch0;
  // the binary32 screen
  int64_t qt32, nc32, ch32;
  // the matrix cores: padded counts, blocks of 512 queries, node chunks of chm (kMfma) or rows of mask words (kCells) per
  // workgroup row, partial rows; their sample of msample nodes, every mstride-th, in ssplit chunks of schunk
  int64_t npad, Mpad, qblocks, nsplit, chm, msample, mstride, ssplit, schunk;
  int mparts, sshift;  // (sshift: a bound's low 16 bits carry the sample position, scaled by it)
  int64_t nres;        // node rows the arena is sized for when it must grow
  // the cell-ordered scan: sub-chunks, mask words over them, sub-chunks padded to whole words
  int nsub, nwords, nsubp;
};

constexpr int64_t kSampleNodes = 16384;

NnPlan plan_nearest(const mjpl_engine *e, int64_t n, int64_t cap, int64_t M, bool have_bound) {
  NnPlan p = {};
  const int nplan = p.nplan = (int)e->qidx.size();
  p.rgridM = (unsigned)((M + kBlock - 1) / kBlock);
  p.path = NnPath::kLds;
  if (nplan > kNNMaxPlan || n <= 0) return p;
  // 2-D decomposition: 512 queries per block x node chunks, then a reduction over the chunks;
  // chunks sized for about eight two-wave blocks per SIMD quartet (the scan is one dependent
  // chain per query: waves, not instructions, hide its latencies)
  const int qblock = kNNQueries * kNNThreads;
  p.qtiles = (M + qblock - 1) / qblock;
  p.nchunks = std::max<int64_t>(1, (8192 + p.qtiles - 1) / p.qtiles);
  p.nchunks = std::min<int64_t>(p.nchunks, (n + kNNThreads - 1) / kNNThreads);
  p.nchunks = std::max<int64_t>(p.nchunks, 1);
  p.chunk = (n + p.nchunks - 1) / p.nchunks;
  p.chunk = (p.chunk + kNNThreads - 1) / kNNThreads * kNNThreads;
  p.nchunks = (n + p.chunk - 1) / p.chunk;
  // partial results: room for twice the chunks of the float64 scan (the screened scan below
  // cuts the nodes up to twice as fine), and one seed row
  p.maxchunks = 2 * (size_t)p.nchunks + 1;
  p.path = NnPath::kPlain;
  // (4 096 queries: the planner's look-up of its tail lanes.  A ranged look-up brings a bound for every query with it -- the
  //  distance already found below the range: screened from 8 192 nodes on.  It still takes the sample of its range: the
  //  nodes a round adds reach into places the tree was far from, and a query there would otherwise park every one of them)
  if (!(M >= 4096 && (n >= 16 * kSampleNodes || (have_bound && n >= 8192)) && nplan >= 2 && nplan <= 9)) return p;
  p.stride = std::max<int64_t>(1, n / kSampleNodes);
  // (chunks of the float64 sample scan: whole multiples of the scan's tile, and never more of them than partial rows --
  //  16 384 / nc0 rounded DOWN gave one chunk too many for some node counts, whose row was the seed row: ADVICE r05)
  p.nc0 = std::min<int64_t>(p.maxchunks, kSampleNodes / kNNThreads);
  p.ch0 = ((kSampleNodes + p.nc0 - 1) / p.nc0 + kNNThreads - 1) / kNNThreads * kNNThreads;
  p.nsamp64 = std::min<int64_t>(kSampleNodes, n / kNNThreads * kNNThreads);  // (a short range: all of it)
  p.nch0 = (p.nsamp64 + p.ch0 - 1) / p.ch0;
  const int qb32 = kNN32Queries * kNNThreads;
  p.qt32 = (M + qb32 - 1) / qb32;
  p.nc32 = std::max<int64_t>(1, (8192 + p.qt32 - 1) / p.qt32);
  p.nc32 = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(p.nc32, (int64_t)p.maxchunks), n / (8 * kNNThreads)));
  p.ch32 = (n + p.nc32 - 1) / p.nc32;
  p.ch32 = (p.ch32 + kNNThreads - 1) / kNNThreads * kNNThreads;
  p.nc32 = (n + p.ch32 - 1) / p.ch32;
  p.path = NnPath::kScreen32;
  // (the matrix-core kernel reads its node tiles through a buffer descriptor with 32-bit offsets: 2^26 nodes at most)
  if (!(e->nn_mfma && nplan <= kNNMMaxPlan && n < ((int64_t)1 << 26))) return p;
  p.Mpad = (M + kNNMQueries - 1) / kNNMQueries * kNNMQueries;
  p.qblocks = p.Mpad / kNNMQueries;
  int64_t sample, row;  // nodes of the strided sample asked for; the arena's node rows are whole multiples of `row`
  if (e->nn_cells && n >= e->nn_cells_min && n >= 64 * kNNCellSub && n < ((int64_t)1 << 25)) {
    p.path = NnPath::kCells;
    sample = e->nn_cells_sample;
    row = kNNCellSub;
    p.npad = (n + row - 1) / row * row;
    p.nsub = (int)(p.npad / kNNCellSub);
    p.nwords = (p.nsub + 63) / 64;
    p.nsubp = p.nwords * 64;
    // (sub-chunks per workgroup row: whole mask words, ~2 048 workgroups in all, no more rows than words)
    p.nsplit = std::max<int64_t>(1, std::min<int64_t>((4096 + p.qblocks - 1) / p.qblocks, p.nwords));
  } else {
    p.path = NnPath::kMfma;
    sample = e->nn_sample;
    row = 32;
    p.npad = (n + row - 1) / row * row;
    p.nsplit = std::max<int64_t>(1, std::min<int64_t>((2048 + p.qblocks - 1) / p.qblocks, n / 4096));
    p.chm = ((n + p.nsplit - 1) / p.nsplit + 31) / 32 * 32;
    p.nsplit = (n + p.chm - 1) / p.chm;
  }
  p.mparts = (int)(2 * p.nsplit);
  // (trees grow call by call, and a reallocation stalls the stream: room for four times the nodes, within the slab)
  // (a planner says how far its trees may grow: nn_reserve_nodes -- no reallocation in the middle of a search)
  p.nres = std::min<int64_t>((cap + row - 1) / row * row, std::max<int64_t>(4 * p.npad, e->nn_reserve_nodes));
  if (p.path == NnPath::kCells) p.nres = std::max<int64_t>(p.npad, p.nres);
  // every query's bound: the sample node the screen likes best, its distance exactly
  p.msample = std::max<int64_t>(32, std::min<int64_t>(sample, n / 16 / 32 * 32));
  p.mstride = std::max<int64_t>(1, n / p.msample);
  // (the sample in as many chunks as give the chip ~1 024 workgroups: a look-up of few queries -- the planner's tail lanes --
  //  would otherwise scan it with eight)
  p.ssplit = std::max<int64_t>(1, std::min<int64_t>((1024 + p.qblocks - 1) / p.qblocks, p.msample / 256));
  p.schunk = ((p.msample + p.ssplit - 1) / p.ssplit + 31) / 32 * 32;
  for (p.sshift = 0; (p.msample >> p.sshift) > 65536; p.sshift++) {}
  return p;
}

// the look-up as the caller gave it: nodes [0, n) of the slab at `nodes` (column stride `cap`); outer_d2 (or NULL): a distance
// every query already has an answer at -- nothing farther is of interest; st: the stream it is enqueued on
struct NnBatch {
  const double *nodes;
  int64_t n, cap;
  const double *queries;
  int64_t M;
  int32_t *out_idx;
  double *out_d2;
  const double *outer_d2;
  hipStream_t st;
};

// pick the <NP> instantiation of a look-up's kernel for the planning dimension, LO..HI
template <int LO, int HI, class F>
int dispatch_nplan(int nplan, F &&f) {
  if constexpr (LO > HI) return fail(MJPL_E_ARG, "nearest: no kernel for %d planning columns", nplan);
  else return nplan == LO ? f(std::integral_constant<int, LO>{}) : dispatch_nplan<LO + 1, HI>(nplan, f);
}

// the partial rows: maxchunks of them and the seed row, distances then indices
struct NnParts {
  double *pd2, *seed_d2;
  int32_t *pidx, *seed_idx;
};

int reserve_parts(NnScratch &s, const NnPlan &p, int64_t M, NnParts *r) {
  MJPL_TRY(s.parts.reserve((p.maxchunks + 1) * (size_t)M * (sizeof(double) + sizeof(int32_t))));
  r->pd2 = (double *)s.parts.p;
  r->seed_d2 = r->pd2 + p.maxchunks * (size_t)M;
  r->pidx = (int32_t *)(r->seed_d2 + (size_t)M);
  r->seed_idx = r->pidx + p.maxchunks * (size_t)M;
  return MJPL_OK;
}

// what the screened scans work on.  Either arena starts with xbits: [0] largest coordinate, [1] wild, [2] largest node
// norm, [3] option "nn_probe" = 2 counts the exact evaluations here (mjpl_nearest_last_screen and "nn_last_exact_pairs"
// read them at offset 0)
struct NnArena {
  unsigned *xbits;
  uint4 *q16, *nodes16;  // the operands: queries (in scan order, kCells) and nodes
  float *qn;
  double *mp_d2;         // the matrix cores' partial rows
  int32_t *mp_idx;
  // kCells
  unsigned *mm;
  NncPlan *plan;
  uint4 *q16u;           // the queries in the callers' order, for the sample
  float *qnu;
  double *queries_s, *bound2_s, *nodes_s;
  float *qf, *q32c, *nbox, *nodes32;
  unsigned *kq_in, *kq_out, *kn_in, *kn_out;
  int32_t *pq_in, *perm_q, *pn_in, *perm_n, *ccount, *clist;
  unsigned long long *masks;
  void *tmpq, *tmpn;
  size_t sort_tmp_q, sort_tmp_n;  // (rocprim's, set before the arena is carved)
};

// kMfma, `nodes` node rows (the node rows last: they are what grows).  (The byte count is the spans' own: a few dozen bytes
// below what was reserved before this listing existed, which added 32 spare bytes to the unrounded sum.)
void carve_mfma(Carver &c, const NnPlan &p, int64_t M, int64_t nodes, NnArena *a) {
  a->xbits = c.take<unsigned>(64);
  a->q16 = c.take<uint4>((size_t)p.Mpad * 4);
  a->mp_d2 = c.take<double>((size_t)p.mparts * M, 8);
  a->qn = c.take<float>((size_t)p.Mpad);
  a->mp_idx = c.take<int32_t>((size_t)p.mparts * M, 32);
  a->nodes16 = c.take<uint4>((size_t)nodes * 2, 32);
}

// kCells, `nodes` node rows (whole sub-chunks): what grows with the tree last -- masks, lists, boxes, keys + permutation
// (in / out), sort space, sorted rows, packed rows
void carve_cells(Carver &c, const NnPlan &p, int64_t M, int64_t nodes, NnArena *a) {
  const size_t waves = (size_t)(p.Mpad / 128), np = (size_t)nodes, words = (size_t)((nodes / kNNCellSub + 63) / 64);
  a->xbits = c.take<unsigned>(64);
  a->mm = c.take<unsigned>(64);
  a->plan = c.take<NncPlan>(1, 512);
  a->q16u = c.take<uint4>((size_t)p.Mpad * 4);
  a->q16 = c.take<uint4>((size_t)p.Mpad * 4);
  a->qnu = c.take<float>((size_t)p.Mpad);
  a->qn = c.take<float>((size_t)p.Mpad);
  a->queries_s = c.take<double>((size_t)8 * M);
  a->bound2_s = c.take<double>((size_t)M);
  a->qf = c.take<float>((size_t)p.Mpad * 8);
  a->q32c = c.take<float>((size_t)p.Mpad * 8);
  a->kq_in = c.take<unsigned>((size_t)M);
  a->kq_out = c.take<unsigned>((size_t)M);
  a->pq_in = c.take<int32_t>((size_t)M);
  a->perm_q = c.take<int32_t>((size_t)M);
  a->mp_d2 = c.take<double>((size_t)p.mparts * M);
  a->mp_idx = c.take<int32_t>((size_t)p.mparts * M);
  a->tmpq = c.take<char>(a->sort_tmp_q);
  a->ccount = c.take<int32_t>(waves);
  a->masks = c.take<unsigned long long>(waves * words);
  a->clist = c.take<int32_t>(waves * words * 64);
  a->nbox = c.take<float>(16 * words * 64);
  a->kn_in = c.take<unsigned>(np);
  a->kn_out = c.take<unsigned>(np);
  a->pn_in = c.take<int32_t>(np);
  a->perm_n = c.take<int32_t>(np);
  a->tmpn = c.take<char>(a->sort_tmp_n);
  a->nodes_s = c.take<double>(8 * np);
  a->nodes16 = c.take<uint4>(np * 2);
  a->nodes32 = c.take<float>(np * 8);
}

// The arena of a screened look-up.  When it must grow it is sized for p.nres node rows: a search that has declared its
// capacity never reallocates in the middle.
int reserve_arena(NnScratch &s, const NnPlan &p, const NnBatch &b, NnArena *a) {
  const bool cells = p.path == NnPath::kCells;
  if (cells) {
    // (rocprim picks its algorithm by the item count: the node sort's space for the count it is sized for AND the one it sorts.
    //  Were its size not monotonic in the count, a later n could ask for more than the arena reserved at nres holds and grow it
    //  in the middle of a search: slower once, never wrong -- the arena is carved anew by every call)
    size_t at_n = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a->sort_tmp_n, (const unsigned *)nullptr, (unsigned *)nullptr, (const int32_t *)nullptr,
                                    (int32_t *)nullptr, (size_t)p.nres, 0, kNNCKeyBits, b.st);
    (void)rocprim::radix_sort_pairs(nullptr, at_n, (const unsigned *)nullptr, (unsigned *)nullptr, (const int32_t *)nullptr,
                                    (int32_t *)nullptr, (size_t)b.n, 0, kNNCKeyBits, b.st);
    a->sort_tmp_n = std::max(a->sort_tmp_n, at_n);
    (void)rocprim::radix_sort_pairs(nullptr, a->sort_tmp_q, (const unsigned *)nullptr, (unsigned *)nullptr, (const int32_t *)nullptr,
                                    (int32_t *)nullptr, (size_t)b.M, 0, 16, b.st);
  }
  auto carve = [&](char *base, int64_t nodes) {
    Carver c{base};
    if (cells) carve_cells(c, p, b.M, nodes, a);
    else carve_mfma(c, p, b.M, nodes, a);
    return c.at;
  };
  if (carve(nullptr, p.npad) > s.arena.cap) MJPL_TRY(s.arena.reserve(carve(nullptr, p.nres)));
  (void)carve(s.arena.p, p.npad);
  return MJPL_OK;
}

// ---- the stages.  Each takes the plan, the scratch it works in (partial rows, arena) and the batch.

// the float64 scan of nodes [0, nn) in chunks of `ch` (stride > 1: a sample; only_if_wild: an arena's xbits, or NULL)
int stage_scan64(const NnPlan &p, const NnParts &r, const NnBatch &b, int64_t nn, int64_t ch, int64_t nch, int64_t stride,
                 const unsigned *only_if_wild) {
  const dim3 grid((unsigned)p.qtiles, (unsigned)nch);
  auto go = [&](auto NP) -> int {
    return launch_kernel(b.st, k_nearest_part<NP()>, grid, kNNThreads, 0, b.nodes, nn, b.cap, b.queries, b.M, p.nplan, ch, r.pidx, r.pd2, stride,
                         only_if_wild);
  };
  if (p.nplan < 2 || p.nplan > 9) return go(std::integral_constant<int, 0>{});  // (any number of columns up to 16)
  return dispatch_nplan<2, 9>(p.nplan, go);
}

// the operands of the matrix cores: node and query rows in binary16 (kCells: the sorted rows of eight, about the centre)
int stage_pack(const NnBatch &b, const double *src, int64_t count, int64_t col_stride, int64_t padded, int nplan, int is_query,
               uint4 *out16, float *nrm, unsigned *xbits, int64_t row_stride, const float *centre) {
  return launch_kernel(b.st, k_nn_pack, dim3((unsigned)((padded + 256 * kNNPackRows - 1) / (256 * kNNPackRows))), 256, 0, src, count, col_stride,
                       padded, nplan, is_query, out16, nrm, xbits, row_stride, centre);
}

// every query's bound (the seed row) from a strided sample of the nodes.  With an arena `a` (kMfma, kCells) the matrix
// cores take it from the sample node the screen likes best -- sample_nodes with column stride sample_pitch, queries
// q16 / qn --; wild coordinates: the float64 scan of the callers' sample; either pair of kernels leaves at once when
// the other serves the call.  Without (kScreen32) the float64 scan is all.  Then never above the callers' own bound.
int stage_bound(const NnPlan &p, const NnParts &r, const NnBatch &b, const NnArena *a, const double *sample_nodes, int64_t sample_pitch,
                const uint4 *q16, const float *qn) {
  const unsigned *xbits = a ? a->xbits : nullptr;
  const bool cells = p.path == NnPath::kCells;
  if (a) {
    NnCells sc{};
    if (cells) {
      sc.pack_idx = 1;
      sc.node_rows = 1;  // (the sorted nodes: rows of eight; the queries still the callers' columns)
      sc.idx_shift = p.sshift;
    }
    const dim3 gs((unsigned)p.qblocks, (unsigned)((p.msample + p.schunk - 1) / p.schunk));
    MJPL_TRY(launch_kernel(b.st, k_nn_fill_inf, dim3(p.rgridM), kBlock, 0, r.seed_d2, b.M, xbits));
    MJPL_TRY(dispatch_nplan<2, kNNMMaxPlan>(p.nplan, [&](auto NP) -> int {
      return launch_kernel(b.st, k_nearest_mfma<NP(), true>, gs, kNNMWaves * 64, 0, sample_nodes, p.msample, sample_pitch, b.queries, b.M,
                           (const uint4 *)a->nodes16, q16, qn, xbits, p.schunk, p.mstride, r.seed_d2, (int32_t *)nullptr, (double *)nullptr, sc);
    }));
  }
  MJPL_TRY(stage_scan64(p, r, b, p.nsamp64, p.ch0, p.nch0, p.stride, xbits));
  MJPL_TRY(launch_kernel(b.st, k_nearest_reduce, dim3(p.rgridM), kBlock, 0, (const int32_t *)r.pidx, (const double *)r.pd2, b.M, (int)p.nch0,
                         r.seed_idx, r.seed_d2, (const int32_t *)nullptr, (const double *)nullptr, xbits));
  if (!b.outer_d2) return MJPL_OK;
  if (cells) return launch_kernel(b.st, k_nnc_bound_min, dim3(p.rgridM), kBlock, 0, r.seed_d2, b.outer_d2, b.M, xbits);
  return launch_kernel(b.st, k_nearest_bound_min, dim3(p.rgridM), kBlock, 0, r.seed_d2, b.outer_d2, b.M);
}

// the binary32 screen over the callers' rows, within the bounds of the seed row (with an arena: wild coordinates only)
int stage_screen32(const NnPlan &p, const NnParts &r, const NnBatch &b, const unsigned *only_if_wild) {
  const dim3 grid((unsigned)p.qt32, (unsigned)p.nc32);
  return dispatch_nplan<2, 9>(p.nplan, [&](auto NP) -> int {
    return launch_kernel(b.st, k_nearest_part32<NP()>, grid, kNNThreads, 0, b.nodes, b.n, b.cap, b.queries, b.M, p.ch32, (const double *)r.seed_d2,
                         r.pidx, r.pd2, only_if_wild);
  });
}

// kCells 1: the nodes along the curve, their boxes, and the operands (the queries' in the callers' order, for the sample)
int stage_cells_order(const NnPlan &p, const NnArena &a, const NnBatch &b) {
  const int64_t n = b.n;
  HIP_TRY(hipMemsetAsync(a.xbits, 0, 16, b.st));
  HIP_TRY(hipMemsetAsync(a.mm, 0xff, 32, b.st));
  HIP_TRY(hipMemsetAsync(a.mm + 8, 0, 32, b.st));
  MJPL_TRY(launch_kernel(b.st, k_nnc_minmax, dim3((unsigned)((n + 256 * kNNCMinmaxRows - 1) / (256 * kNNCMinmaxRows))), 256, 0, b.nodes, n, b.cap,
                         p.nplan, a.mm));
  MJPL_TRY(launch_kernel(b.st, k_nnc_plan, dim3(1), 64, 0, (const unsigned *)a.mm, p.nplan, a.plan));
  MJPL_TRY(launch_kernel(b.st, k_nnc_keys, dim3((unsigned)((n + 255) / 256)), 256, 0, b.nodes, n, b.cap, p.nplan, (const NncPlan *)a.plan, a.kn_in,
                         a.pn_in));
  size_t tn = a.sort_tmp_n;
  if (rocprim::radix_sort_pairs(a.tmpn, tn, (const unsigned *)a.kn_in, a.kn_out, (const int32_t *)a.pn_in, a.perm_n, (size_t)n, 0, kNNCKeyBits,
                                b.st) != hipSuccess)
    return fail(MJPL_E_HIP, "nearest: sorting the nodes failed");
  MJPL_TRY(launch_kernel(b.st, k_nnc_gather, dim3((unsigned)((p.npad + 255) / 256)), 256, 0, b.nodes, b.cap, (const int32_t *)a.perm_n, n, p.npad,
                         p.nplan, a.nodes_s, a.nodes32, (const NncPlan *)a.plan));
  MJPL_TRY(launch_kernel(b.st, k_nnc_boxes, dim3((unsigned)((p.nsub + 3) / 4)), 256, 0, (const double *)a.nodes_s, n, p.nplan, p.nsub, p.nsubp,
                         a.nbox));
  MJPL_TRY(stage_pack(b, a.nodes_s, n, 1, p.npad, p.nplan, 0, a.nodes16, nullptr, a.xbits, 8, a.plan->ctr));
  return stage_pack(b, b.queries, b.M, b.M, p.Mpad, p.nplan, 1, a.q16u, a.qnu, a.xbits, 1, a.plan->ctr);
}

// kCells 3, 4: the queries in scan order (by where on the curve the bound was found), every wave's candidate sub-chunks,
// the scan of those
int stage_cells_scan(mjpl_engine *e, const NnPlan &p, const NnParts &r, const NnArena &a, const NnBatch &b) {
  const int64_t M = b.M;
  MJPL_TRY(launch_kernel(b.st, k_nnc_query_keys, dim3(p.rgridM), kBlock, 0, (const double *)r.seed_d2, M, a.kq_in, a.pq_in));
  size_t tq = a.sort_tmp_q;
  if (rocprim::radix_sort_pairs(a.tmpq, tq, (const unsigned *)a.kq_in, a.kq_out, (const int32_t *)a.pq_in, a.perm_q, (size_t)M, 0, 16, b.st) !=
      hipSuccess)
    return fail(MJPL_E_HIP, "nearest: sorting the queries failed");
  MJPL_TRY(launch_kernel(b.st, k_nnc_gather_queries, dim3((unsigned)((p.Mpad + kBlock - 1) / kBlock)), kBlock, 0, b.queries, (const double *)r.seed_d2,
                         (const int32_t *)a.perm_q, M, p.Mpad, p.nplan, a.queries_s, a.bound2_s, a.qf, a.q32c, (const NncPlan *)a.plan));
  MJPL_TRY(stage_pack(b, a.queries_s, M, 1, p.Mpad, p.nplan, 1, a.q16, a.qn, a.xbits, 8, a.plan->ctr));
  if (e->nn_home)
    MJPL_TRY(launch_kernel(b.st, k_nnc_home, dim3((unsigned)((M + 255) / 256)), 256, 0, (const double *)a.nodes_s, b.n, (const double *)a.queries_s, M,
                           p.nplan, p.mstride, p.sshift, p.nsub, a.bound2_s, a.qf, (const unsigned *)a.xbits));
  const unsigned waves = (unsigned)(p.Mpad / 128);
  MJPL_TRY(launch_kernel(b.st, k_nn_candidates, dim3(waves, (unsigned)((p.nwords + 3) / 4)), 256, 0, (const float *)a.qf, M, (const float *)a.nbox,
                         p.nsub, p.nsubp, p.nwords, a.masks, (const unsigned *)a.xbits));
  MJPL_TRY(launch_kernel(b.st, k_nn_compact, dim3((waves + 3) / 4), 256, 0, (const unsigned long long *)a.masks, p.nwords, (int)waves, a.clist,
                         (int64_t)p.nsubp, a.ccount, (const unsigned *)a.xbits));
  NnCells cs{};
  cs.list = a.clist; cs.count = a.ccount; cs.perm_n = a.perm_n; cs.list_pitch = p.nsubp; cs.probe = e->nn_probe; cs.counter = a.xbits + 3;
  cs.node_rows = 1; cs.query_rows = 1; cs.nodes32 = a.nodes32; cs.queries32 = a.q32c; cs.second = e->nn_second_screen;
  const dim3 gm(waves, (unsigned)p.nsplit);  // (one wave of 128 queries per workgroup)
  kt_mark(e, 2, b.st);
  MJPL_TRY(dispatch_nplan<2, kNNMMaxPlan>(p.nplan, [&](auto NP) -> int {
    return launch_kernel(b.st, k_nearest_mfma<NP(), false, true>, gm, 64, 0, (const double *)a.nodes_s, b.n, p.npad, (const double *)a.queries_s, M,
                         (const uint4 *)a.nodes16, (const uint4 *)a.q16, (const float *)a.qn, (const unsigned *)a.xbits, (int64_t)0, (int64_t)1,
                         a.bound2_s, a.mp_idx, a.mp_d2, cs);
  }));
  kt_mark(e, 2, b.st);
  return MJPL_OK;
}

// kMfma: the operands, then (behind the bounds) the scan of all nodes in chunks of chm
int stage_mfma_pack(const NnPlan &p, const NnArena &a, const NnBatch &b) {
  HIP_TRY(hipMemsetAsync(a.xbits, 0, 12, b.st));
  MJPL_TRY(stage_pack(b, b.nodes, b.n, b.cap, p.npad, p.nplan, 0, a.nodes16, nullptr, a.xbits, 1, nullptr));
  return stage_pack(b, b.queries, b.M, b.M, p.Mpad, p.nplan, 1, a.q16, a.qn, a.xbits, 1, nullptr);
}

int stage_mfma_scan(const NnPlan &p, const NnParts &r, const NnArena &a, const NnBatch &b) {
  const dim3 gm((unsigned)p.qblocks, (unsigned)p.nsplit);
  return dispatch_nplan<2, kNNMMaxPlan>(p.nplan, [&](auto NP) -> int {
    return launch_kernel(b.st, k_nearest_mfma<NP(), false>, gm, kNNMWaves * 64, 0, b.nodes, b.n, b.cap, b.queries, b.M, (const uint4 *)a.nodes16,
                         (const uint4 *)a.q16, (const float *)a.qn, (const unsigned *)a.xbits, p.chm, (int64_t)1, r.seed_d2, a.mp_idx, a.mp_d2,
                         NnCells{});
  });
}

// One look-up on scratch `s`, enqueued on b.st.  The launches per path (plan_nearest), in order; (w): returns at once
// unless some coordinate was wild, (m): unless none was:
//   kLds       k_nearest
//   kPlain     part                                                                                       reduce
//   kScreen32  bound [part of the sample, reduce, bound_min]                                      part32  reduce
//   kMfma      pack x2  bound [fill_inf, mfma<sample> (m), part (w), reduce (w), bound_min]  mfma (m)  part32 (w)  reduce_ties
//   kCells     minmax, plan, keys, sort, gather, boxes, pack x2  bound [as kMfma, nnc_bound_min]  query_keys, sort,
//              gather_queries, pack, (home), candidates, compact, | mfma<cells> (m) |  part32 (w)  nnc_reduce
// (|: the kernel_timer's class 2 brackets the cell-ordered scan.)  What s.last says is set before anything is enqueued.
int nearest_core(mjpl_engine *e, NnScratch &s, const NnBatch &b) {
  HIP_TRY(hipSetDevice(e->device));
  s.last = {};
  const NnPlan p = plan_nearest(e, b.n, b.cap, b.M, b.outer_d2 != nullptr);
  if (p.path == NnPath::kLds) {
    MJPL_TRY(launch_kernel(b.st, k_nearest, dim3(p.rgridM), kBlock, 2 * (size_t)p.nplan * kBlock * sizeof(double), b.nodes, b.n, b.cap, b.queries, b.M,
                           p.nplan, b.out_idx, b.out_d2));
    HIP_TRY(hipGetLastError());
    return MJPL_OK;
  }
  NnParts r;
  MJPL_TRY(reserve_parts(s, p, b.M, &r));
  const int32_t *parts_idx = r.pidx;
  const double *parts_d2 = r.pd2;
  if (p.path == NnPath::kPlain) {
    MJPL_TRY(stage_scan64(p, r, b, b.n, p.chunk, p.nchunks, 1, nullptr));
    MJPL_TRY(launch_kernel(b.st, k_nearest_reduce, dim3(p.rgridM), kBlock, 0, parts_idx, parts_d2, b.M, (int)p.nchunks, b.out_idx, b.out_d2,
                           (const int32_t *)nullptr, (const double *)nullptr, (const unsigned *)nullptr));
  } else if (p.path == NnPath::kScreen32) {
    s.last.path = 1;
    MJPL_TRY(stage_bound(p, r, b, nullptr, nullptr, 0, nullptr, nullptr));
    MJPL_TRY(stage_screen32(p, r, b, nullptr));
    MJPL_TRY(launch_kernel(b.st, k_nearest_reduce, dim3(p.rgridM), kBlock, 0, parts_idx, parts_d2, b.M, (int)p.nc32, b.out_idx, b.out_d2,
                           (const int32_t *)nullptr, (const double *)nullptr, (const unsigned *)nullptr));
  } else {
    s.last.path = 2;
    s.last.cells = p.path == NnPath::kCells;
    NnArena a = {};
    MJPL_TRY(reserve_arena(s, p, b, &a));
    if (s.last.cells) {
      s.last.count_at = (size_t)((char *)a.ccount - s.arena.p);
      s.last.waves = (int)((b.M + 127) / 128);
      s.last.nsub = p.nsub;
      MJPL_TRY(stage_cells_order(p, a, b));
      MJPL_TRY(stage_bound(p, r, b, &a, a.nodes_s, p.npad, a.q16u, a.qnu));
      MJPL_TRY(stage_cells_scan(e, p, r, a, b));
      MJPL_TRY(stage_screen32(p, r, b, a.xbits));
      // the answers in the callers' order
      MJPL_TRY(launch_kernel(b.st, k_nnc_reduce, dim3(p.rgridM), kBlock, 0, (const int32_t *)a.mp_idx, (const double *)a.mp_d2, b.M, p.mparts,
                             (const int32_t *)a.perm_q, b.out_idx, b.out_d2, (const unsigned *)a.xbits, parts_idx, parts_d2, (int)p.nc32));
    } else {
      MJPL_TRY(stage_mfma_pack(p, a, b));
      MJPL_TRY(stage_bound(p, r, b, &a, b.nodes, b.cap, a.q16, a.qn));
      MJPL_TRY(stage_mfma_scan(p, r, a, b));
      MJPL_TRY(stage_screen32(p, r, b, a.xbits));
      MJPL_TRY(launch_kernel(b.st, k_nearest_reduce_ties, dim3(p.rgridM), kBlock, 0, (const int32_t *)a.mp_idx, (const double *)a.mp_d2, b.M, p.mparts,
                             b.out_idx, b.out_d2, (const unsigned *)a.xbits, parts_idx, parts_d2, (int)p.nc32));
    }
  }
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// the look-up over the node range [n0, n) behind an answer (outer_idx, outer_d2: NULL = none) for the nodes below n0
int nearest_range(mjpl_engine *e, NnScratch &s, hipStream_t st, const double *dnodes, int64_t n0, int64_t n, int64_t cap, const double *dqueries,
                  int64_t M, int32_t *dout_idx, double *dout_dist2, const int32_t *outer_idx, const double *outer_d2) {
  if (n0 == 0 && !outer_idx) return nearest_core(e, s, {dnodes, n, cap, dqueries, M, dout_idx, dout_dist2, nullptr, st});
  if (n0 < 0 || n0 > n || (outer_idx && !outer_d2)) return fail(MJPL_E_ARG, "nearest_range: bad range");
  HIP_TRY(hipSetDevice(e->device));
  s.last = {};
  double *d2 = dout_dist2;
  if (!d2) {
    MJPL_TRY(s.spare.reserve((size_t)M));
    d2 = s.spare.p;
  }
  if (n > n0) MJPL_TRY(nearest_core(e, s, {dnodes + n0, n - n0, cap, dqueries, M, dout_idx, d2, outer_idx ? outer_d2 : nullptr, st}));
  MJPL_TRY(launch_kernel(st, k_nearest_rebase, dim3((unsigned)((M + kBlock - 1) / kBlock)), kBlock, 0, M, n0, n > n0 ? 1 : 0, dout_idx, d2, dout_dist2,
                         outer_idx, outer_d2));
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// ---- push configurations out to a minimum clearance (mjpl_push.h)
namespace {

// Argument checks of mjpl_push_out*: check_common, the ranges of the descriptor (NaN refused everywhere), lo <= hi per
// planning column, every output non-null when N > 0.
int check_push_args(const mjpl_engine *e, const mjpl_push_desc *d, const void *Q, int64_t N, int layout,
                    std::initializer_list<const void *> outs) {
  MJPL_TRY(check_common(e, Q, N, layout));
  if (!d) return fail(MJPL_E_ARG, "mjpl_push_out: NULL descriptor");
  if (!(d->d_min > 0)) return fail(MJPL_E_ARG, "d_min must be > 0 (NaN is refused), got %g", d->d_min);
  if (!(d->overshoot >= 0)) return fail(MJPL_E_ARG, "overshoot must be >= 0 (NaN is refused), got %g", d->overshoot);
  if (!(d->damping > 0)) return fail(MJPL_E_ARG, "damping must be > 0 (NaN is refused), got %g", d->damping);
  if (!(d->step_max > 0)) return fail(MJPL_E_ARG, "step_max must be > 0 (NaN is refused), got %g", d->step_max);
  if (d->max_iter < 1) return fail(MJPL_E_ARG, "max_iter must be >= 1, got %d", d->max_iter);
  if (d->max_pairs < 1) return fail(MJPL_E_ARG, "max_pairs must be >= 1, got %d", d->max_pairs);
  for (size_t k = 0; k < e->qidx.size(); k++) {
    const double lo = d->lo ? d->lo[k] : -INFINITY, hi = d->hi ? d->hi[k] : INFINITY;
    if (!(lo <= hi)) return fail(MJPL_E_ARG, "bounds of planning column %d: lo %g, hi %g (NaN and lo > hi are refused)", (int)k, lo, hi);
  }
  if (N > 0)
    for (const void *o : outs)
      if (!o) return fail(MJPL_E_ARG, "NULL output pointer");
  return MJPL_OK;
}

// The loop of mjpl_push_out* on device pointers (include/mjpl_hip.h states the iteration).  Per chunk of at most
// kContactRows rows: gather into work buffer 0, then per iteration one k_distance<DM_NEAR> launch over the active
// rows, one k_push_step launch, and one 4-byte read of the other buffer's fill counter, which sizes the next
// iteration (0: the chunk is done).  Then one k_distance<DM_CLEAR> launch over Q_out and the status rule.
int launch_push(mjpl_engine *e, const mjpl_push_desc &d, const double *dQ, int64_t N, int layout, double *dQ_out,
                double *dclear, int32_t *dpair, int32_t *diters, int32_t *dstatus) {
  MJPL_TRY(check_pair_types(e));
  const int nplan = (int)e->qidx.size(), K = d.max_pairs;
  if (nplan < 1 || nplan > kPushMaxPlan)
    return fail(MJPL_E_CAPACITY, "mjpl_push_out: %d planning columns (1..%d supported)", nplan, kPushMaxPlan);
  const double dstar = d.d_min + e->ct_margin_max;
  const hipStream_t st = e->stream;
  if (!e->h_push_n) HIP_TRY(hipHostMalloc((void **)&e->h_push_n, sizeof(int)));
  // scratch of a chunk: doubles = 2 work buffers [rows][nplan], dist [rows][K], grad [rows][K][nplan];
  // ints = 2 id lists [rows], count [rows], pair and status [rows][K], then the two counters
  const size_t rows = (size_t)std::min<int64_t>(N, kContactRows), rk = rows * (size_t)K, rn = rows * (size_t)nplan;
  MJPL_TRY(e->d_push_f64.reserve(2 * rn + rk + rk * nplan));
  MJPL_TRY(e->d_push_i32.reserve(3 * rows + 2 * rk + 2));
  double *work[2] = {e->d_push_f64.p, e->d_push_f64.p + rn};
  double *ndist = work[1] + rn, *ngrad = ndist + rk;
  int *ids[2] = {e->d_push_i32.p, e->d_push_i32.p + rows};
  int *ncount = ids[1] + rows, *npair = ncount + rows, *nstatus = npair + rk, *ctr = nstatus + rk;

  // every row starts as its own answer: Q_out = Q, iters 0, no flag
  HIP_TRY(hipMemcpyAsync(dQ_out, dQ, (size_t)N * nplan * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemsetAsync(diters, 0, (size_t)N * sizeof(int32_t), st));
  HIP_TRY(hipMemsetAsync(dstatus, 0, (size_t)N * sizeof(int32_t), st));

  for (int64_t i0 = 0; i0 < N; i0 += (int64_t)rows) {
    int n = (int)std::min<int64_t>((int64_t)rows, N - i0);
    hipLaunchKernelGGL(k_push_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dQ, N, i0, n, nplan, layout,
                       work[0], ids[0]);
    HIP_TRY(hipGetLastError());
    for (int it = 0; it < d.max_iter && n > 0; it++) {
      const int cur = it & 1, nxt = cur ^ 1;
      MJPL_TRY(launch_distance(e, DM_NEAR, work[cur], n, MJPL_AOS, dstar, ndist, nullptr, npair, ngrad, nullptr, nullptr,
                               nstatus, K, ncount));
      HIP_TRY(hipMemsetAsync(ctr + nxt, 0, sizeof(int), st));
      PushStep a = {};
      a.rows = work[cur]; a.ids = ids[cur]; a.n = n;
      a.next_rows = work[nxt]; a.next_ids = ids[nxt]; a.next_n = ctr + nxt;
      a.K = K; a.count = ncount; a.pair = npair; a.slot_status = nstatus; a.dist = ndist; a.grad = ngrad;
      a.cd = e->d_ct_dp;
      a.d_min = d.d_min; a.overshoot = d.overshoot; a.damping = d.damping; a.step_max = d.step_max;
      a.it = it; a.last = it + 1 == d.max_iter;
      a.Q_out = dQ_out; a.N = N; a.i0 = i0; a.layout = layout; a.iters = diters; a.flag = dstatus;
      MJPL_TRY(dispatch_nplan<1, kPushMaxPlan>(nplan, [&](auto NP) -> int {
        PushBounds<NP()> bd;
        for (int k = 0; k < NP(); k++) {
          bd.lo[k] = d.lo ? d.lo[k] : -INFINITY;
          bd.hi[k] = d.hi ? d.hi[k] : INFINITY;
        }
        hipLaunchKernelGGL(k_push_step<NP()>, dim3((unsigned)((n + kPushBlock - 1) / kPushBlock)), dim3(kPushBlock), 0, st, a, bd);
        HIP_TRY(hipGetLastError());
        return MJPL_OK;
      }));
      if (a.last) break;
      HIP_TRY(hipMemcpyAsync(e->h_push_n, ctr + nxt, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      n = *e->h_push_n;
    }
  }
  MJPL_TRY(launch_distance(e, DM_CLEAR, dQ_out, N, layout, dstar, nullptr, dclear, dpair));
  hipLaunchKernelGGL(k_push_status, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, dclear, d.d_min, dstatus);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

}  // namespace

// ---- time-optimal path parameterisation (mjpl_topp.h)
namespace {

// first grid point of path b (the host's topp_g_off)
int64_t topp_g_off_h(const int64_t *wp_off, int G, int64_t b) { return (int64_t)G * (wp_off[b] - b) + b; }

// Argument checks of a batch of paths, shared by mjpl_topp_* and mjpl_jerk_*: the engine, the batch size and the columns ...
int check_path_dims(const mjpl_engine *e, const void *desc, int64_t B, int nq) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  if (!desc) return fail(MJPL_E_ARG, "mjpl_topp: NULL descriptor");
  if (B < 0 || B > INT32_MAX) return fail(MJPL_E_ARG, "mjpl_topp: batch size %lld out of range", (long long)B);
  if (nq < 1 || nq > kToppMaxCols) return fail(MJPL_E_CAPACITY, "mjpl_topp: %d columns (1..%d supported)", nq, kToppMaxCols);
  return MJPL_OK;
}

// ... and the offsets and non-null batches
int check_path_batches(int grid, const void *W, const int64_t *wp_off, int64_t B, std::initializer_list<const void *> bufs) {
  if (B == 0) return MJPL_OK;
  if (!wp_off) return fail(MJPL_E_ARG, "mjpl_topp: NULL offsets");
  if (wp_off[0] != 0) return fail(MJPL_E_ARG, "wp_off[0] must be 0, got %lld", (long long)wp_off[0]);
  for (int64_t b = 0; b < B; b++) {
    const int64_t n = wp_off[b + 1] - wp_off[b];
    if (n < 2) return fail(MJPL_E_ARG, "path %lld has %lld waypoints (offsets must rise by at least 2)", (long long)b, (long long)n);
    if (n > (1 << 24) / grid) return fail(MJPL_E_CAPACITY, "path %lld: %lld waypoints at grid %d exceed 2^24 grid points", (long long)b, (long long)n, grid);
  }
  if (!W) return fail(MJPL_E_ARG, "NULL batch pointer");
  for (const void *o : bufs)
    if (!o) return fail(MJPL_E_ARG, "NULL batch pointer");
  return MJPL_OK;
}

// Argument checks shared by mjpl_topp_profile* and mjpl_topp_sample*: the descriptor, the offsets, non-null batches.
int check_topp_args(const mjpl_engine *e, const mjpl_topp_desc *d, const void *W, const int64_t *wp_off, int64_t B,
                    std::initializer_list<const void *> bufs) {
  MJPL_TRY(check_path_dims(e, d, B, d ? d->nq : 0));
  if (d->grid < 2 || d->grid > (1 << 16)) return fail(MJPL_E_ARG, "grid must be 2..65536 intervals per segment, got %d", d->grid);
  if (!d->vmin || !d->vmax || !d->amin || !d->amax) return fail(MJPL_E_ARG, "mjpl_topp: NULL limit array");
  for (int j = 0; j < d->nq; j++) {
    if (!(d->vmin[j] < 0 && d->vmax[j] > 0 && d->vmin[j] > -INFINITY && d->vmax[j] < INFINITY))
      return fail(MJPL_E_ARG, "velocity limits of column %d: [%g, %g] (finite vmin < 0 < vmax wanted, NaN is refused)", j, d->vmin[j], d->vmax[j]);
    if (!(d->amin[j] < 0 && d->amax[j] > 0 && d->amin[j] > -INFINITY && d->amax[j] < INFINITY))
      return fail(MJPL_E_ARG, "acceleration limits of column %d: [%g, %g] (finite amin < 0 < amax wanted, NaN is refused)", j, d->amin[j], d->amax[j]);
  }
  return check_path_batches(d->grid, W, wp_off, B, bufs);
}

// The call's tables on the device: [wp_off | samp_off] and the limits.  The stream is drained first: an earlier call's
// launches read the same buffers.
int topp_upload(mjpl_engine *e, int nq, std::initializer_list<const double *> lims, const int64_t *wp_off, const int64_t *samp_off,
                int64_t B) {
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t nb = (size_t)B + 1, nd = nq;
  e->topp_off_h.assign(2 * nb, 0);
  std::copy(wp_off, wp_off + nb, e->topp_off_h.begin());
  if (samp_off) std::copy(samp_off, samp_off + nb, e->topp_off_h.begin() + nb);
  e->topp_lim_h.clear();
  for (const double *l : lims) e->topp_lim_h.insert(e->topp_lim_h.end(), l, l + nd);  // (at most four arrays)
  MJPL_TRY(e->d_topp_off.reserve(2 * nb, 1024));
  MJPL_TRY(e->d_topp_lim.reserve(4 * kToppMaxCols));
  HIP_TRY(hipMemcpyAsync(e->d_topp_off.p, e->topp_off_h.data(), 2 * nb * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
  HIP_TRY(hipMemcpyAsync(e->d_topp_lim.p, e->topp_lim_h.data(), e->topp_lim_h.size() * sizeof(double), hipMemcpyHostToDevice, e->stream));
  return MJPL_OK;
}

// c' of the Thomas recurrence on the device, for the longest of these paths (k_topp_spline reads it; the stream is drained)
int topp_cp_table(mjpl_engine *e, const int64_t *wp_off, int64_t B) {
  int64_t nmax = 0;
  for (int64_t b = 0; b < B; b++) nmax = std::max(nmax, wp_off[b + 1] - wp_off[b]);
  if ((size_t)nmax > e->topp_cp_h.size()) {  // c'[0] = 0, c'[k] = 1 / (4 - c'[k-1])
    e->topp_cp_h.assign(std::max<size_t>(nmax, 1024), 0.0);
    for (size_t k = 1; k < e->topp_cp_h.size(); k++) e->topp_cp_h[k] = 1.0 / (4.0 - e->topp_cp_h[k - 1]);
    MJPL_TRY(e->d_topp_cp.reserve(e->topp_cp_h.size()));
    HIP_TRY(hipMemcpyAsync(e->d_topp_cp.p, e->topp_cp_h.data(), e->topp_cp_h.size() * sizeof(double), hipMemcpyHostToDevice,
                           e->stream));
  }
  return MJPL_OK;
}

// mjpl_topp_profile* on device batches (wp_off on the host): the spline of every path in one launch, then per chunk of
// paths whose workspace fits the option "topp_chunk_bytes" (always at least one path) the two grid kernels and the sweeps.
int launch_topp_profile(mjpl_engine *e, const mjpl_topp_desc &d, const double *dW, const int64_t *wp_off, int64_t B, double *dM,
                        double *dx, double *du, double *dt, int32_t *dstatus) {
  e->topp_last_chunks = 0;
  MJPL_TRY(topp_upload(e, d.nq, {d.vmin, d.vmax, d.amin, d.amax}, wp_off, nullptr, B));
  const hipStream_t st = e->stream;
  const size_t chunk_bytes = (size_t)e->topp_chunk_bytes;
  MJPL_TRY(topp_cp_table(e, wp_off, B));
  ToppBatch a = {};
  a.W = dW; a.wp_off = e->d_topp_off.p; a.B = (int)B; a.d = d.nq; a.G = d.grid;
  a.lim = e->d_topp_lim.p; a.cp = e->d_topp_cp.p; a.M = dM;
  a.x = dx; a.u = du; a.t = dt; a.status = dstatus;
  hipLaunchKernelGGL(k_topp_spline, dim3((unsigned)((B * d.nq + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  const size_t rows = 2 * (size_t)d.nq, per_pt = (5 * rows + 1) * sizeof(double);
  for (int64_t b0 = 0; b0 < B;) {
    const int64_t g0 = topp_g_off_h(wp_off, d.grid, b0);
    int64_t b1 = b0 + 1;
    while (b1 < B && (size_t)(topp_g_off_h(wp_off, d.grid, b1 + 1) - g0) * per_pt <= chunk_bytes) b1++;
    const int64_t pts = topp_g_off_h(wp_off, d.grid, b1) - g0;
    MJPL_TRY(e->d_topp_ws.reserve((size_t)pts * (5 * rows + 1)));
    const size_t span = (size_t)pts * rows;
    a.b0 = (int)b0; a.b1 = (int)b1; a.g0 = g0; a.pts = pts;
    a.wP = e->d_topp_ws.p; a.wrho = a.wP + span; a.wpp = a.wrho + span; a.wg = a.wpp + span; a.ws = a.wg + span;
    a.wK = a.ws + span;
    const dim3 grid((unsigned)((span + 255) / 256));
    hipLaunchKernelGGL(k_topp_lines, grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_topp_pairs, grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_topp_sweep, dim3((unsigned)((b1 - b0 + kToppSweepWaves - 1) / kToppSweepWaves)), dim3(64 * kToppSweepWaves), 0, st, a);
    HIP_TRY(hipGetLastError());
    e->topp_last_chunks++;
    b0 = b1;
  }
  return MJPL_OK;
}

int check_topp_sample_args(const int64_t *wp_off, int64_t B, double dt, const int64_t *samp_off) {
  if (!(dt > 0) || !(dt < INFINITY)) return fail(MJPL_E_ARG, "dt must be > 0 and finite (NaN is refused), got %g", dt);
  if (B == 0) return MJPL_OK;
  if (!samp_off) return fail(MJPL_E_ARG, "mjpl_topp_sample: NULL offsets");
  if (samp_off[0] != 0) return fail(MJPL_E_ARG, "samp_off[0] must be 0, got %lld", (long long)samp_off[0]);
  for (int64_t b = 0; b < B; b++)
    if (samp_off[b + 1] < samp_off[b]) return fail(MJPL_E_ARG, "samp_off falls at path %lld", (long long)b);
  return MJPL_OK;
}

int launch_topp_sample(mjpl_engine *e, const mjpl_topp_desc &d, const double *dW, const int64_t *wp_off, int64_t B,
                       const double *dM, const double *dx, const double *du, const double *dt_grid, double dt,
                       const int64_t *samp_off, double *dpos, double *dvel, double *dacc) {
  MJPL_TRY(topp_upload(e, d.nq, {d.vmin, d.vmax, d.amin, d.amax}, wp_off, samp_off, B));
  ToppSamples a = {};
  a.W = dW; a.M = dM; a.x = dx; a.u = du; a.t = dt_grid;
  a.wp_off = e->d_topp_off.p; a.samp_off = e->d_topp_off.p + (B + 1);
  a.B = (int)B; a.d = d.nq; a.G = d.grid; a.dt = dt;
  a.pos = dpos; a.vel = dvel; a.acc = dacc;
  hipLaunchKernelGGL(k_topp_sample, dim3((unsigned)((samp_off[B] + 255) / 256)), dim3(256), 0, e->stream, a);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// ---- jerk-limited path parameterisation (mjpl_jerk.h); offsets, limits and the spline go the way of mjpl_topp_*
// Argument checks shared by mjpl_jerk_profile* and mjpl_jerk_sample*
int check_jerk_args(const mjpl_engine *e, const mjpl_jerk_desc *d, const void *W, const int64_t *wp_off, int64_t B,
                    std::initializer_list<const void *> bufs) {
  MJPL_TRY(check_path_dims(e, d, B, d ? d->nq : 0));
  if (d->grid < 1 || d->grid > (1 << 16)) return fail(MJPL_E_ARG, "grid must be 1..65536 intervals per segment, got %d", d->grid);
  if (!d->vlim || !d->alim || !d->jlim) return fail(MJPL_E_ARG, "mjpl_jerk: NULL limit array");
  for (int j = 0; j < d->nq; j++)
    if (!(d->vlim[j] > 0 && d->vlim[j] < INFINITY && d->alim[j] > 0 && d->alim[j] < INFINITY && d->jlim[j] > 0 && d->jlim[j] < INFINITY))
      return fail(MJPL_E_ARG, "limits of column %d: velocity %g, acceleration %g, jerk %g (finite magnitudes > 0 wanted, NaN is refused)", j,
                  d->vlim[j], d->alim[j], d->jlim[j]);
  return check_path_batches(d->grid, W, wp_off, B, bufs);
}

// mjpl_jerk_profile* on device batches (wp_off on the host): five launches for the whole batch, no workspace
int launch_jerk_profile(mjpl_engine *e, const mjpl_jerk_desc &d, const double *dW, const int64_t *wp_off, int64_t B, double *dM,
                        double *dlim, double *dv, double *dvp, double *dtc, double *dt, int32_t *dstatus) {
  MJPL_TRY(topp_upload(e, d.nq, {d.vlim, d.alim, d.jlim}, wp_off, nullptr, B));
  const hipStream_t st = e->stream;
  MJPL_TRY(topp_cp_table(e, wp_off, B));
  ToppBatch s = {};
  s.W = dW; s.wp_off = e->d_topp_off.p; s.B = (int)B; s.d = d.nq; s.cp = e->d_topp_cp.p; s.M = dM;
  hipLaunchKernelGGL(k_topp_spline, dim3((unsigned)((B * d.nq + 255) / 256)), dim3(256), 0, st, s);
  HIP_TRY(hipGetLastError());
  JerkBatch a = {};
  a.W = dW; a.wp_off = e->d_topp_off.p; a.B = (int)B; a.d = d.nq; a.G = d.grid;
  a.lim = e->d_topp_lim.p; a.M = dM; a.pts = topp_g_off_h(wp_off, d.grid, B);
  a.L = dlim; a.v = dv; a.vp = dvp; a.tc = dtc; a.t = dt; a.status = dstatus;
  const dim3 per_path((unsigned)((B + kJerkSweepWaves - 1) / kJerkSweepWaves)), waves(64 * kJerkSweepWaves);
  hipLaunchKernelGGL(k_jerk_bounds, dim3((unsigned)((a.pts * 16 + 255) / 256)), dim3(256), 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_jerk_sweep, per_path, waves, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_jerk_intervals, dim3((unsigned)((a.pts + kJerkSweepWaves - 1) / kJerkSweepWaves)), waves, 0, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_jerk_times, per_path, waves, 0, st, a);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

int launch_jerk_sample(mjpl_engine *e, const mjpl_jerk_desc &d, const double *dW, const int64_t *wp_off, int64_t B, const double *dM,
                       const double *dlim, const double *dv, const double *dvp, const double *dtc, const double *dt_grid, double dt,
                       const int64_t *samp_off, double *dpos, double *dvel, double *dacc) {
  MJPL_TRY(topp_upload(e, d.nq, {d.vlim, d.alim, d.jlim}, wp_off, samp_off, B));
  JerkSamples a = {};
  a.W = dW; a.M = dM; a.L = dlim; a.v = dv; a.vp = dvp; a.tc = dtc; a.t = dt_grid;
  a.wp_off = e->d_topp_off.p; a.samp_off = e->d_topp_off.p + (B + 1);
  a.B = (int)B; a.d = d.nq; a.G = d.grid; a.dt = dt;
  a.pos = dpos; a.vel = dvel; a.acc = dacc;
  hipLaunchKernelGGL(k_jerk_sample, dim3((unsigned)((samp_off[B] + 255) / 256)), dim3(256), 0, e->stream, a);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// ---- path shortcutting (mjpl_shortcut.h)
int check_shortcut_args(const mjpl_engine *e, const mjpl_shortcut_desc *d, const void *W, const int64_t *wp_off, int64_t B,
                        const void *keep, const void *n_out, const void *status) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  if (!d) return fail(MJPL_E_ARG, "mjpl_shortcut: NULL descriptor");
  if (B < 0 || B > INT32_MAX) return fail(MJPL_E_ARG, "mjpl_shortcut: batch size %lld out of range", (long long)B);
  if (!(d->step_dist > 0.0)) return fail(MJPL_E_ARG, "`step_dist` must be > 0, got %g", d->step_dist);
  if (!(d->min_saving >= 0.0)) return fail(MJPL_E_ARG, "`min_saving` must be >= 0, got %g", d->min_saving);
  if (d->rounds < 1) return fail(MJPL_E_ARG, "`rounds` must be >= 1, got %d", d->rounds);
  if (d->candidates < 1 || d->candidates > kShortcutLanes)
    return fail(MJPL_E_ARG, "`candidates` must be 1..%d, got %d", kShortcutLanes, d->candidates);
  if (B == 0) return MJPL_OK;
  if (!wp_off) return fail(MJPL_E_ARG, "mjpl_shortcut: NULL offsets");
  if (wp_off[0] != 0) return fail(MJPL_E_ARG, "wp_off[0] must be 0, got %lld", (long long)wp_off[0]);
  for (int64_t b = 0; b < B; b++) {
    const int64_t n = wp_off[b + 1] - wp_off[b];
    if (n < 2) return fail(MJPL_E_ARG, "path %lld has %lld waypoints (offsets must rise by at least 2)", (long long)b, (long long)n);
    if (n > kShortcutMaxRows) return fail(MJPL_E_CAPACITY, "path %lld: %lld waypoints (at most %d supported)", (long long)b, (long long)n, kShortcutMaxRows);
  }
  if (!W || !keep || !n_out || !status) return fail(MJPL_E_ARG, "NULL batch pointer");
  return MJPL_OK;
}

// ---- what mjpl_shortcut_paths*, mjpl_plan_paths*, mjpl_plan_paths_constrained* and the roadmap calls share on the host

// option "kernel_timer" & 1 around one phase of such a call: its first and last event (launch_configs marks events of
// its own between them), for the sums of the call.  A phase is logged only when both of its own events were recorded:
// the pool stops at 4096 events, and later phases go untimed.
using PhaseLog = std::vector<std::array<int, 3>>;

struct PhaseScope {
  mjpl_engine *e;
  PhaseLog &log;
  int phase, at;
  PhaseScope(mjpl_engine *e_, PhaseLog &log_, int phase_) : e(e_), log(log_), phase(phase_), at(e_->kt_used[0]) {
    kt_mark(e, 1, e->stream);
  }
  ~PhaseScope() {
    const int before = e->kt_used[0];
    kt_mark(e, 1, e->stream);
    if (at < before && e->kt_used[0] == before + 1) log.push_back({phase, at, before});
  }
};

// ... and the sums: device time per phase, added to the family's `*_last_ms`
int phase_sums(mjpl_engine *e, const PhaseLog &phases, double *sums) {
  if (phases.empty()) return MJPL_OK;
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (const auto &ph : phases) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e->kt_ev[0][(size_t)ph[1]], e->kt_ev[0][(size_t)ph[2]]));
    sums[ph[0]] += ms;
  }
  return MJPL_OK;
}

// every `*_last_*` value of a family, the times included: at the top of its launchers, and by its entry points on an
// empty batch
void shortcut_reset(mjpl_engine *e) {
  e->shortcut_last_chunks = e->shortcut_last_rounds = e->shortcut_last_edges = 0;
  for (double &ms : e->shortcut_last_ms) ms = 0.0;
}

void plan_reset(mjpl_engine *e) {
  e->plan_last_chunks = e->plan_last_rounds = e->plan_last_edges = 0;
  for (double &ms : e->plan_last_ms) ms = 0.0;
}

void roadmap_reset(mjpl_engine *e) {
  e->roadmap_last_edges = e->roadmap_last_chunks = e->roadmap_last_sweeps = 0;
  for (double &ms : e->roadmap_last_ms) ms = 0.0;
}

// The header the kernels of a round (or of a roadmap query) leave for the host, three words: the bits of the longest edge
// (a double), the edge count, and the problems still at work (the roadmap query: its sweeps).
struct RoundHead {
  double longest;
  int64_t edges;
  int64_t live;
};

inline double head_length(unsigned long long bits) {
  double len;
  memcpy(&len, &bits, sizeof(double));
  return len;
}

inline RoundHead decode_head(const unsigned long long (&w)[3]) { return {head_length(w[0]), (int64_t)w[1], (int64_t)w[2]}; }

// ... read: one small copy and one synchronisation of the engine's stream
int read_head(mjpl_engine *e, const unsigned long long *dhead, RoundHead *h) {
  unsigned long long w[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(w, dhead, sizeof(w), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  *h = decode_head(w);
  return MJPL_OK;
}

// A handful of LONG edges (path shortcutting, smooth_path: planning/utils.py:9-87) is better served by the two
// persistent kernels, which keep every 32nd exact waypoint as a checkpoint: the fused kernel rebuilds an undecided
// waypoint by the recurrence from the start of its edge (measured: 64 edges of 2 400 waypoints 3.9 vs 7.6 ms).  Every
// caller of launch_edges that knows its longest edge asks here, so the same edges take the same kernels whoever asks.
constexpr int64_t kFewEdges = 4096;
inline bool few_long_edges(int64_t E, double longest, double step_dist) { return E <= kFewEdges && longest > 64.0 * step_dist; }

// rocPRIM's space for a scan of n ints (never 0 bytes: a span of the arena, and a null space asks rocPRIM for the size)
int scan_space(hipStream_t st, size_t n, size_t *bytes) {
  *bytes = 0;
  if (rocprim::exclusive_scan(nullptr, *bytes, (int *)nullptr, (int *)nullptr, 0, n, rocprim::plus<int>(), st) != hipSuccess)
    return fail(MJPL_E_HIP, "rocprim::exclusive_scan: no size for %zu counts", n);
  *bytes = std::max<size_t>(*bytes, 1);
  return MJPL_OK;
}

// An arena reserved for a listing of its spans (carve_shortcut and the like), then carved: the listing runs without a
// base for the byte count and with it for the pointers.  An arena that is large enough is left as it is.
template <class List>
int carve_arena(DevBuf<char> &arena, List &&list) {
  Carver size{nullptr};
  list(size);
  MJPL_TRY(arena.reserve(size.at));
  Carver c{arena.p};
  list(c);
  return MJPL_OK;
}

// What the round loop itself touches of a chunk's workspace: the header, the edge counts [counts] and their offsets, the
// scan's space, the round's edge batch and its verdicts.  (The kernels reach the same spans through their batch struct.)
struct RoundSpans {
  unsigned long long *head;
  int *cnt, *off;
  size_t counts;
  void *scan;
  size_t scan_bytes;
  const double *QA, *QB;
  uint8_t *valid;
};

// The rounds [first, last) of one chunk, for the three launchers in lockstep.  Per round: the header is zeroed and the
// launcher proposes, propose(r), both in phase 0; project(r) is what a launcher's propose stage launches after that,
// under phase scopes of its own (constrained planning: project and count) -- then the header is read (read_head).  No
// problem at work ends the chunk's rounds.  A round with edges has them scanned and gathered (phase 0), validated by
// ONE launch_edges (phase 1); commit(have_verdicts) runs in every round (phase 2).  A round before 0 (planning: the
// direct edges) does not count in `rounds`.
template <class Propose, class Project, class Gather, class Commit>
int run_rounds(mjpl_engine *e, PhaseLog &phases, const RoundSpans &s, int first, int last, double step_dist, int64_t *rounds, int64_t *edges,
               Propose &&propose, Project &&project, Gather &&gather, Commit &&commit) {
  const hipStream_t st = e->stream;
  size_t scan_bytes = s.scan_bytes;
  for (int r = first; r < last; r++) {
    {
      PhaseScope ph(e, phases, 0);
      HIP_TRY(hipMemsetAsync(s.head, 0, 3 * sizeof(unsigned long long), st));
      MJPL_TRY(propose(r));
    }
    MJPL_TRY(project(r));
    RoundHead h;
    MJPL_TRY(read_head(e, s.head, &h));
    if (h.live == 0) break;  // every problem of the chunk is retired
    if (r >= 0) ++*rounds;
    if (h.edges > 0) {
      {
        PhaseScope ph(e, phases, 0);
        if (rocprim::exclusive_scan(s.scan, scan_bytes, s.cnt, s.off, 0, s.counts, rocprim::plus<int>(), st) != hipSuccess)
          return fail(MJPL_E_HIP, "rocprim::exclusive_scan failed");
        MJPL_TRY(gather());
      }
      PhaseScope ph(e, phases, 1);
      MJPL_TRY(launch_edges(e, s.QA, s.QB, h.edges, step_dist, MJPL_AOS, 0, s.valid, nullptr, few_long_edges(h.edges, h.longest, step_dist)));
      *edges += h.edges;
    }
    PhaseScope ph(e, phases, 2);
    MJPL_TRY(commit(h.edges > 0 ? 1 : 0));
  }
  return MJPL_OK;
}

// a kernel of these launchers on a stream, with the launch's error
template <class K, class... A>
int launch_checked(hipStream_t st, K kern, dim3 grid, dim3 block, size_t lds, const A &...args) {
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// The workspace of a chunk of `nb` paths with `rows` waypoints between them, K candidates a path.  (The edge batch starts
// on a 256-byte boundary, as the staged batches of mjpl_check_edges do: every span does.)
void carve_shortcut(Carver &c, size_t rows, size_t nb, size_t K, size_t np, size_t scan_bytes, ShortcutBatch *a, RoundSpans *s) {
  const size_t L64 = kShortcutLanes, emax = nb * K;
  a->L = c.take<double>(rows);
  a->cs = c.take<double>(nb * L64);
  a->QA = c.take<double>(emax * np);
  a->QB = c.take<double>(emax * np);
  a->live = c.take<int>(rows);
  a->m = c.take<int>(nb);
  a->state = c.take<int>(nb);
  a->nprop = c.take<int>(nb);
  a->nacc = c.take<int>(nb);
  a->cnt = c.take<int>(nb + 1);
  a->off = c.take<int>(nb + 1);
  a->ci = c.take<int>(nb * L64);
  a->cj = c.take<int>(nb * L64);
  a->crank = c.take<int>(nb * L64);
  uint8_t *valid = c.take<uint8_t>(emax);
  a->valid = valid;
  *s = {a->head, a->cnt, a->off, nb + 1, c.take<char>(scan_bytes), scan_bytes, a->QA, a->QB, valid};
}

// mjpl_shortcut_paths* on device batches (wp_off on the host).  Per chunk of paths whose workspace fits the option
// "shortcut_chunk_bytes" (always at least one path): k_shortcut_init, the chunk's rounds (run_rounds), k_shortcut_finish.
// A round that proposed nothing still commits, without verdicts.
int launch_shortcut(mjpl_engine *e, const mjpl_shortcut_desc &d, const double *dW, const int64_t *wp_off, int64_t B, uint8_t *dkeep,
                    int32_t *dn_out, double *dlength, int32_t *dstatus, int32_t *dproposed, int32_t *daccepted) {
  shortcut_reset(e);
  const hipStream_t st = e->stream;
  HIP_TRY(hipStreamSynchronize(st));  // (an earlier call's launches read the same buffers)
  MJPL_TRY(e->d_sc_off.reserve((size_t)B + 1, 1024));
  MJPL_TRY(e->d_sc_head.reserve(4));
  HIP_TRY(hipMemcpyAsync(e->d_sc_off.p, wp_off, ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  const size_t np = e->qidx.size(), K = (size_t)d.candidates, L64 = kShortcutLanes;
  // what one path adds to a chunk: K edges (two rows and a verdict each), its candidates, its rows' live list and arc lengths
  const size_t per_path = K * (2 * np * sizeof(double) + 1) + L64 * (3 * sizeof(int) + sizeof(double)) + 6 * sizeof(int);
  const size_t per_row = sizeof(int) + sizeof(double), chunk_bytes = (size_t)e->shortcut_chunk_bytes;
  PhaseLog phases;
  ShortcutBatch a = {};
  a.W = dW; a.wp_off = e->d_sc_off.p; a.d = (int)np; a.K = d.candidates;
  a.min_saving = d.min_saving;
  a.seed_mixed = shortcut_mix(d.seed);
  a.head = e->d_sc_head.p;
  a.keep = dkeep; a.n_out = dn_out; a.length = dlength; a.status = dstatus; a.proposed = dproposed; a.accepted = daccepted;
  for (int64_t b0 = 0; b0 < B;) {
    int64_t b1 = b0 + 1;
    size_t bytes = per_path + (size_t)(wp_off[b1] - wp_off[b0]) * per_row;
    while (b1 < B) {
      const size_t more = per_path + (size_t)(wp_off[b1 + 1] - wp_off[b1]) * per_row;
      if (bytes + more > chunk_bytes || (size_t)(b1 - b0 + 1) * K > ((size_t)1 << 30)) break;  // (edge offsets are ints)
      bytes += more;
      b1++;
    }
    const size_t nb = (size_t)(b1 - b0), rows = (size_t)(wp_off[b1] - wp_off[b0]);
    size_t scan_bytes = 0;
    MJPL_TRY(scan_space(st, nb + 1, &scan_bytes));
    RoundSpans s = {};
    MJPL_TRY(carve_arena(e->d_sc_arena, [&](Carver &c) { carve_shortcut(c, rows, nb, K, np, scan_bytes, &a, &s); }));
    a.b0 = (int)b0; a.nb = (int)nb; a.row0 = wp_off[b0];
    const dim3 grid((unsigned)((nb + kShortcutWaves - 1) / kShortcutWaves)), block(64 * kShortcutWaves);
    MJPL_TRY(launch_checked(st, k_shortcut_init, grid, block, 0, a));
    MJPL_TRY(run_rounds(
        e, phases, s, 0, d.rounds, d.step_dist, &e->shortcut_last_rounds, &e->shortcut_last_edges,
        [&](int r) {
          a.round = r;
          return launch_checked(st, k_shortcut_propose, grid, block, 0, a);
        },
        [](int) { return MJPL_OK; },
        [&] {
          a.have_verdicts = 1;  // (a round that gathers has edges)
          return launch_checked(st, k_shortcut_gather, grid, block, 0, a);
        },
        [&](int have_verdicts) {
          a.have_verdicts = have_verdicts;
          return launch_checked(st, k_shortcut_commit, grid, block, 0, a);
        }));
    HIP_TRY(hipMemsetAsync(dkeep + wp_off[b0], 0, rows, st));
    MJPL_TRY(launch_checked(st, k_shortcut_finish, grid, block, 0, a));
    e->shortcut_last_chunks++;
    b0 = b1;
  }
  // an edge the edge kernels refuse counts as invalid here: the pipeline's status word is not this call's to report
  HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), st));
  return phase_sums(e, phases, e->shortcut_last_ms);
}

// ---- planning in lockstep (mjpl_plan.h)
int check_plan_args(const mjpl_engine *e, const mjpl_plan_desc *d, const void *QI, const void *QG, int64_t B, const double *lo,
                    const double *hi, const void *P, const void *n_out, const void *status) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  if (!d) return fail(MJPL_E_ARG, "mjpl_plan: NULL descriptor");
  if (B < 0 || B > INT32_MAX) return fail(MJPL_E_ARG, "mjpl_plan: batch size %lld out of range", (long long)B);
  if (!(d->epsilon > 0.0)) return fail(MJPL_E_ARG, "`epsilon` must be > 0, got %g", d->epsilon);
  if (!(d->step_dist > 0.0)) return fail(MJPL_E_ARG, "`step_dist` must be > 0, got %g", d->step_dist);
  if (d->rounds < 1 || d->rounds > 4096) return fail(MJPL_E_ARG, "`rounds` must be 1..4096, got %d", d->rounds);
  if (d->candidates < 1 || d->candidates > kPlanLanes)
    return fail(MJPL_E_ARG, "`candidates` must be 1..%d, got %d", kPlanLanes, d->candidates);
  if (d->nodes < 2 || d->nodes > 65536) return fail(MJPL_E_ARG, "`nodes` must be 2..65536, got %d", d->nodes);
  if (!lo || !hi) return fail(MJPL_E_ARG, "mjpl_plan: NULL sampling box");
  for (size_t c = 0; c < e->qidx.size(); c++) {
    if (!std::isfinite(lo[c]) || !std::isfinite(hi[c]) || !std::isfinite(hi[c] - lo[c]))
      return fail(MJPL_E_ARG, "sampling box column %zu is not finite: [%g, %g]", c, lo[c], hi[c]);
    if (lo[c] > hi[c]) return fail(MJPL_E_ARG, "sampling box column %zu: lo %g > hi %g", c, lo[c], hi[c]);
  }
  if (B == 0) return MJPL_OK;
  if (!QI || !QG || !P || !n_out || !status) return fail(MJPL_E_ARG, "NULL batch pointer");
  return MJPL_OK;
}

// The workspace of a chunk of `nb` problems with trees of N nodes and `emax` edges a round at most.  The verdicts are one
// span under two names: the ends' first (`end_verdicts` bytes), every round's after.  (The configuration and edge
// batches start on 256-byte boundaries, as the staged batches of mjpl_check_edges do: every span does.)
void carve_plan(Carver &c, size_t nb, size_t emax, size_t end_verdicts, size_t N, size_t np, size_t scan_bytes, PlanBatch *a, RoundSpans *s) {
  const size_t L64 = kPlanLanes;
  a->T = c.take<double>(nb * 2 * N * np);
  a->ct = c.take<double>(nb * np * L64);
  a->cfg = c.take<double>(2 * nb * np);
  a->QA = c.take<double>(emax * np);
  a->QB = c.take<double>(emax * np);
  a->par = c.take<int>(nb * 2 * N);
  a->ck = c.take<int>(nb * L64);
  a->n = c.take<int>(2 * nb);
  a->state = c.take<int>(nb);
  a->gained = c.take<int>(nb);
  a->rused = c.take<int>(nb);
  a->nedges = c.take<int>(nb);
  a->conn = c.take<int>(3 * nb);
  a->jn = c.take<int>(2 * nb);
  a->cnt = c.take<int>(nb + 1);
  a->off = c.take<int>(nb + 1);
  uint8_t *valid = c.take<uint8_t>(std::max(emax, end_verdicts));
  a->cvalid = valid;
  a->valid = valid;
  *s = {a->head, a->cnt, a->off, nb + 1, c.take<char>(scan_bytes), scan_bytes, a->QA, a->QB, valid};
}

// mjpl_plan_paths* on device batches (lo, hi on the host).  Per chunk of problems whose workspace fits the option
// "plan_chunk_bytes" (always at least one problem): k_plan_init, ONE launch_configs on the ends, the chunk's rounds
// (run_rounds) -- the direct edges are round -1 -- then k_plan_finish.
int launch_plan(mjpl_engine *e, const mjpl_plan_desc &d, const double *dQI, const double *dQG, int64_t B, const double *lo,
                const double *hi, double *dP, int32_t *dn_out, int32_t *dstatus, int32_t *drounds_used, int32_t *dedges,
                int32_t *dtree_nodes) {
  plan_reset(e);
  const hipStream_t st = e->stream;
  HIP_TRY(hipStreamSynchronize(st));  // (an earlier call's launches read the same buffers)
  const size_t np = e->qidx.size(), K = (size_t)d.candidates, N = (size_t)d.nodes, L64 = kPlanLanes;
  MJPL_TRY(e->d_pl_box.reserve(2 * np, 64));
  MJPL_TRY(e->d_pl_head.reserve(4));
  HIP_TRY(hipMemcpyAsync(e->d_pl_box.p, lo, np * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->d_pl_box.p + np, hi, np * sizeof(double), hipMemcpyHostToDevice, st));
  const size_t prows = (size_t)d.rounds + 2;
  HIP_TRY(hipMemsetAsync(dP, 0, (size_t)B * prows * np * sizeof(double), st));
  // what one problem adds to a chunk: two trees with their parents, K + 1 edges (two rows and a verdict each), the
  // round's targets and the nodes they step from, its two ends, its counters
  const size_t per_problem = 2 * N * (np * sizeof(double) + sizeof(int)) + (K + 1) * (2 * np * sizeof(double) + 1) +
                             L64 * (np * sizeof(double) + sizeof(int)) + 2 * np * sizeof(double) + 16 * sizeof(int);
  const size_t fit = std::max<size_t>((size_t)e->plan_chunk_bytes / per_problem, 1);
  const size_t chunk = std::min(fit, ((size_t)1 << 30) / (K + 1));  // (edge offsets are ints)
  PhaseLog phases;
  PlanBatch a = {};
  a.QI = dQI; a.QG = dQG; a.box = e->d_pl_box.p;
  a.d = (int)np; a.K = d.candidates; a.N = d.nodes; a.R = d.rounds;
  a.epsilon = d.epsilon;
  a.seed_mixed = shortcut_mix(d.seed);
  a.head = e->d_pl_head.p;
  a.P = dP; a.n_out = dn_out; a.status = dstatus; a.rounds_used = drounds_used; a.edges = dedges; a.tree_nodes = dtree_nodes;
  for (int64_t b0 = 0; b0 < B; b0 += (int64_t)chunk) {
    const size_t nb = std::min(chunk, (size_t)(B - b0));
    size_t scan_bytes = 0;
    MJPL_TRY(scan_space(st, nb + 1, &scan_bytes));
    RoundSpans s = {};
    MJPL_TRY(carve_arena(e->d_pl_arena, [&](Carver &c) { carve_plan(c, nb, nb * (K + 1), 2 * nb, N, np, scan_bytes, &a, &s); }));
    a.b0 = (int)b0; a.nb = (int)nb;
    const dim3 grid((unsigned)((nb + kPlanWaves - 1) / kPlanWaves)), block(64 * kPlanWaves);
    MJPL_TRY(launch_checked(st, k_plan_init, grid, block, 0, a));
    MJPL_TRY(launch_configs(e, a.cfg, (int64_t)(2 * nb), MJPL_AOS, s.valid, nullptr));
    // (a problem at work has at least one edge: no round here goes without validation)
    MJPL_TRY(run_rounds(
        e, phases, s, -1, d.rounds, d.step_dist, &e->plan_last_rounds, &e->plan_last_edges,
        [&](int r) {
          a.round = r;
          return launch_checked(st, k_plan_propose, grid, block, 0, a);
        },
        [](int) { return MJPL_OK; },
        [&] { return launch_checked(st, k_plan_gather, grid, block, 0, a); },
        [&](int) { return launch_checked(st, k_plan_commit, grid, block, 0, a); }));
    MJPL_TRY(launch_checked(st, k_plan_finish, grid, block, 0, a));
    e->plan_last_chunks++;
  }
  // an edge the edge kernels refuse counts as invalid here: the pipeline's status word is not this call's to report
  HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), st));
  return phase_sums(e, phases, e->plan_last_ms);
}

// ---- roadmap planning (mjpl_roadmap.h)
constexpr int64_t kRoadmapMaxNodes = (int64_t)1 << 20, kRoadmapMaxProblems = (int64_t)1 << 24;

int check_roadmap_common(const mjpl_engine *e, const void *d, double radius, double step_dist, int64_t N) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  if (!d) return fail(MJPL_E_ARG, "mjpl_roadmap: NULL descriptor");
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(MJPL_E_ARG, "`radius` must be > 0 and finite, got %g", radius);
  if (!(step_dist > 0.0) || !std::isfinite(step_dist)) return fail(MJPL_E_ARG, "`step_dist` must be > 0 and finite, got %g", step_dist);
  if (N < 0 || N > kRoadmapMaxNodes) return fail(MJPL_E_ARG, "mjpl_roadmap: %lld nodes (0..2^20 supported)", (long long)N);
  if (rm_knn_lds((int)e->qidx.size()) > ((size_t)64 << 10))
    return fail(MJPL_E_CAPACITY, "mjpl_roadmap: %zu planning columns do not fit the neighbour kernel's LDS", e->qidx.size());
  return MJPL_OK;
}

int check_roadmap_build_args(const mjpl_engine *e, const mjpl_roadmap_desc *d, const void *Q, int64_t N, const void *node_valid,
                             const void *row_off, const void *adj, const void *w) {
  MJPL_TRY(check_roadmap_common(e, d, d ? d->radius : 1.0, d ? d->step_dist : 1.0, N));
  if (d->k < 1 || d->k > kRmMaxK) return fail(MJPL_E_ARG, "`k` must be 1..%d, got %d", kRmMaxK, d->k);
  if (N == 0) return MJPL_OK;
  if (!Q || !node_valid || !row_off || !adj || !w) return fail(MJPL_E_ARG, "NULL batch pointer");
  return MJPL_OK;
}

int check_roadmap_query_args(const mjpl_engine *e, const mjpl_roadmap_query_desc *d, const void *Q, int64_t N, const void *node_valid,
                             const void *row_off, const void *adj, const void *w, const void *QI, const void *QG, int64_t B,
                             const void *P, const void *n_out, const void *status) {
  MJPL_TRY(check_roadmap_common(e, d, d ? d->radius : 1.0, d ? d->step_dist : 1.0, N));
  if (d->connections < 1 || d->connections > kRmMaxK) return fail(MJPL_E_ARG, "`connections` must be 1..%d, got %d", kRmMaxK, d->connections);
  if (d->max_rows < 2) return fail(MJPL_E_ARG, "`max_rows` must be at least 2, got %d", d->max_rows);
  if (B < 0 || B > kRoadmapMaxProblems) return fail(MJPL_E_ARG, "mjpl_roadmap_query: batch size %lld out of range", (long long)B);
  if (!row_off || (N > 0 && (!Q || !node_valid || !adj || !w))) return fail(MJPL_E_ARG, "NULL graph pointer");
  if (B == 0) return MJPL_OK;
  if (!QI || !QG || !P || !n_out || !status) return fail(MJPL_E_ARG, "NULL batch pointer");
  return MJPL_OK;
}

inline unsigned rm_grid(size_t n) { return (unsigned)((n + kRmBlock - 1) / kRmBlock); }

// rocPRIM's space for a radix sort of n keys (bits 0 .. 52: a node index is below 2^21) and a scan of n ints
int roadmap_space(hipStream_t st, size_t n, size_t *bytes) {
  size_t sort_bytes = 0, scan_bytes = 0;
  if (rocprim::radix_sort_keys(nullptr, sort_bytes, (unsigned long long *)nullptr, (unsigned long long *)nullptr, n, 0, 53, st) != hipSuccess)
    return fail(MJPL_E_HIP, "rocprim: no size for %zu keys", n);
  MJPL_TRY(scan_space(st, n, &scan_bytes));
  *bytes = std::max(sort_bytes, scan_bytes);
  return MJPL_OK;
}

// The workspace of a build of N nodes with M = N k neighbour slots, `batch` edges to a launch: the finite rows, the
// neighbour lists, the edge batch; flags and their positions; the sort keys (in, out) and the candidate pairs; rocPRIM's space
struct RmBuildSpans {
  double *cfg, *nn_d2, *QA, *QB;
  int *nn_j, *nn_cnt, *flag, *pos;
  uint8_t *fin, *evalid;
  unsigned long long *ka, *kb, *pairs;
  void *tmp;
};

void carve_roadmap_build(Carver &c, size_t N, size_t M, size_t batch, size_t np, size_t tmp_bytes, RmBuildSpans *w) {
  w->cfg = c.take<double>(N * np);
  w->nn_d2 = c.take<double>(M);
  w->QA = c.take<double>(batch * np);
  w->QB = c.take<double>(batch * np);
  w->nn_j = c.take<int>(M);
  w->nn_cnt = c.take<int>(N);
  w->flag = c.take<int>(M + 1);
  w->pos = c.take<int>(M + 1);
  w->fin = c.take<uint8_t>(N);
  w->evalid = c.take<uint8_t>(M);
  w->ka = c.take<unsigned long long>(2 * M);
  w->kb = c.take<unsigned long long>(2 * M);
  w->pairs = c.take<unsigned long long>(M);
  w->tmp = c.take<char>(tmp_bytes);
}

// The workspace of a query of B problems with C connections an end and `emax` edges at most; `dist`: distances of the
// searches that do not keep theirs in LDS (0: none, the batch's pointer stays null).  What the host code writes through
// and the kernels only read comes back in `w`.
struct RmQuerySpans {
  double *cfg;
  uint8_t *fin, *cvalid, *evalid;
  int *att_j, *att_cnt;
  double *att_d2;
  void *tmp;
};

void carve_roadmap_query(Carver &c, size_t B, size_t C, size_t emax, size_t dist, size_t np, size_t tmp_bytes, RmQuery *a, RmQuerySpans *w) {
  w->cfg = c.take<double>(2 * B * np);
  a->att_d2 = w->att_d2 = c.take<double>(2 * B * C);
  a->dist = dist ? c.take<double>(dist) : nullptr;
  a->QA = c.take<double>(emax * np);
  a->QB = c.take<double>(emax * np);
  a->att_j = w->att_j = c.take<int>(2 * B * C);
  a->att_cnt = w->att_cnt = c.take<int>(2 * B);
  a->state = c.take<int>(B);
  a->cnt = c.take<int>(B + 1);
  a->off = c.take<int>(B + 1);
  a->fin = w->fin = c.take<uint8_t>(B);
  a->cvalid = w->cvalid = c.take<uint8_t>(2 * B);
  a->valid = w->evalid = c.take<uint8_t>(emax);
  w->tmp = c.take<char>(tmp_bytes);
}

int roadmap_knn(mjpl_engine *e, const RmKnn &a) {
  if (a.M == 0) return MJPL_OK;
  hipLaunchKernelGGL(k_rm_knn, dim3((unsigned)((a.M + kRmTile - 1) / kRmTile)), dim3(kRmTile), rm_knn_lds(a.d), e->stream, a);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

// mjpl_roadmap_build* on device arrays: k_rm_finite, ONE launch_configs, the neighbour lists, the candidate pairs by a
// sort, one synchronisation (their number, then the longest edge of every launch), launch_edges per chunk of the option
// "roadmap_chunk_bytes", the directed keys by a second sort, the CSR.
int launch_roadmap_build(mjpl_engine *e, const mjpl_roadmap_desc &d, const double *dQ, int64_t N64, uint8_t *dnode_valid,
                         int32_t *drow_off, int32_t *dadj, double *dw) {
  roadmap_reset(e);
  const hipStream_t st = e->stream;
  HIP_TRY(hipStreamSynchronize(st));  // (an earlier call's launches read the same buffers)
  const size_t np = e->qidx.size(), N = (size_t)N64, k = (size_t)d.k, M = N * k;
  const unsigned long long none = (unsigned long long)N << 32;
  // one launch's edges: two rows and a verdict each
  const size_t chunk = std::min<size_t>(std::max<size_t>((size_t)e->roadmap_chunk_bytes / (2 * np * sizeof(double) + 1), 1), (size_t)1 << 30);
  size_t tmp_bytes = 0;
  MJPL_TRY(roadmap_space(st, 2 * M + 1, &tmp_bytes));
  RmBuildSpans w = {};
  MJPL_TRY(carve_arena(e->d_rm_arena, [&](Carver &c) { carve_roadmap_build(c, N, M, std::min(chunk, M), np, tmp_bytes, &w); }));
  PhaseLog phases;
  {
    PhaseScope ph(e, phases, 0);
    hipLaunchKernelGGL(k_rm_finite, dim3(rm_grid(N)), dim3(kRmBlock), 0, st, dQ, (const double *)nullptr, (int)N, (int)np, w.cfg, w.fin);
    HIP_TRY(hipGetLastError());
    MJPL_TRY(launch_configs(e, w.cfg, (int64_t)N, MJPL_AOS, dnode_valid, nullptr));
    hipLaunchKernelGGL(k_rm_mask, dim3(rm_grid(N)), dim3(kRmBlock), 0, st, dnode_valid, (const uint8_t *)w.fin, (int)N);
    HIP_TRY(hipGetLastError());
  }
  int E32 = 0;
  {
    PhaseScope ph(e, phases, 1);
    RmKnn a = {};
    a.X = dQ; a.xok = dnode_valid; a.M = (int)N; a.Q = dQ; a.qok = dnode_valid; a.N = (int)N; a.d = (int)np; a.k = d.k;
    a.r2 = d.radius * d.radius; a.lo2 = a.r2 * 0x1.0p-40; a.self = 1;
    a.nn_j = w.nn_j; a.nn_d2 = w.nn_d2; a.nn_cnt = w.nn_cnt;
    MJPL_TRY(roadmap_knn(e, a));
    hipLaunchKernelGGL(k_rm_pair_keys, dim3(rm_grid(M)), dim3(kRmBlock), 0, st, (const int32_t *)w.nn_j, (int64_t)M, d.k, none, w.ka);
    HIP_TRY(hipGetLastError());
    if (rocprim::radix_sort_keys(w.tmp, tmp_bytes, w.ka, w.kb, M, 0, 53, st) != hipSuccess) return fail(MJPL_E_HIP, "rocprim::radix_sort_keys failed");
    hipLaunchKernelGGL(k_rm_unique, dim3(rm_grid(M + 1)), dim3(kRmBlock), 0, st, (const unsigned long long *)w.kb, (int64_t)M, none, w.flag);
    HIP_TRY(hipGetLastError());
    if (rocprim::exclusive_scan(w.tmp, tmp_bytes, w.flag, w.pos, 0, M + 1, rocprim::plus<int>(), st) != hipSuccess)
      return fail(MJPL_E_HIP, "rocprim::exclusive_scan failed");
    hipLaunchKernelGGL(k_rm_compact, dim3(rm_grid(M)), dim3(kRmBlock), 0, st, (const unsigned long long *)w.kb, (int64_t)M, (const int *)w.flag,
                       (const int *)w.pos, w.pairs);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(&E32, w.pos + M, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const size_t E = (size_t)E32, nchunks = (E + chunk - 1) / chunk;
  e->roadmap_last_edges = (int64_t)E;
  if (E > 0) {
    std::vector<unsigned long long> longest(nchunks);
    {
      PhaseScope ph(e, phases, 2);
      MJPL_TRY(e->d_rm_head.reserve(nchunks, 64));
      HIP_TRY(hipMemsetAsync(e->d_rm_head.p, 0, nchunks * sizeof(unsigned long long), st));
      hipLaunchKernelGGL(k_rm_longest, dim3(rm_grid(E)), dim3(kRmBlock), 0, st, (const unsigned long long *)w.pairs, (int64_t)E, (int64_t)chunk, dQ,
                         (int)np, e->d_rm_head.p);
      HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(longest.data(), e->d_rm_head.p, nchunks * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t c = 0; c < nchunks; c++) {
      const size_t e0 = c * chunk, ne = std::min(chunk, E - e0);
      const bool long_edges = few_long_edges((int64_t)ne, head_length(longest[c]), d.step_dist);
      PhaseScope ph(e, phases, 2);
      hipLaunchKernelGGL(k_rm_edge_rows, dim3(rm_grid(ne * np)), dim3(kRmBlock), 0, st, (const unsigned long long *)w.pairs, (int64_t)e0, (int64_t)ne, dQ,
                         (int)np, w.QA, w.QB);
      HIP_TRY(hipGetLastError());
      MJPL_TRY(launch_edges(e, w.QA, w.QB, (int64_t)ne, d.step_dist, MJPL_AOS, 0, w.evalid + e0, nullptr, long_edges));
      e->roadmap_last_chunks++;
    }
  }
  {
    PhaseScope ph(e, phases, 3);
    if (E > 0) {
      hipLaunchKernelGGL(k_rm_dir_keys, dim3(rm_grid(E)), dim3(kRmBlock), 0, st, (const unsigned long long *)w.pairs, (const uint8_t *)w.evalid, (int64_t)E,
                         none, w.ka);
      HIP_TRY(hipGetLastError());
      if (rocprim::radix_sort_keys(w.tmp, tmp_bytes, w.ka, w.kb, 2 * E, 0, 53, st) != hipSuccess) return fail(MJPL_E_HIP, "rocprim::radix_sort_keys failed");
    }
    hipLaunchKernelGGL(k_rm_row_off, dim3(rm_grid(N + 1)), dim3(kRmBlock), 0, st, (const unsigned long long *)w.kb, (int64_t)(2 * E), (int)N, drow_off);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_rm_csr, dim3(rm_grid(2 * M)), dim3(kRmBlock), 0, st, (const unsigned long long *)w.kb, (int64_t)(2 * E), (int64_t)(2 * M), none, dQ,
                       (int)np, dadj, dw);
    HIP_TRY(hipGetLastError());
  }
  // an edge the edge kernels refuse counts as invalid here: the pipeline's status word is not this call's to report
  HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), st));
  return phase_sums(e, phases, e->roadmap_last_ms);
}

// mjpl_roadmap_query* on device arrays: k_rm_finite on the ends, ONE launch_configs, the attachments, one synchronisation
// (the edge count and the longest edge), ONE launch_edges, then k_rm_search: one launch when the distances fit in LDS,
// otherwise one per chunk of problems whose workspace fits the option "roadmap_chunk_bytes".
int launch_roadmap_query(mjpl_engine *e, const mjpl_roadmap_query_desc &d, const double *dQ, int64_t N64, const uint8_t *dnode_valid,
                         const int32_t *drow_off, const int32_t *dadj, const double *dw, const double *dQI, const double *dQG, int64_t B64,
                         double *dP, int32_t *dn_out, int32_t *dstatus, double *dcost) {
  roadmap_reset(e);
  const hipStream_t st = e->stream;
  HIP_TRY(hipStreamSynchronize(st));  // (an earlier call's launches read the same buffers)
  const size_t np = e->qidx.size(), N = (size_t)N64, B = (size_t)B64, C = (size_t)d.connections, emax = B * (1 + 2 * C);
  int lds_max = 0;
  HIP_TRY(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, e->device));
  const bool in_lds = N <= (size_t)e->roadmap_lds_nodes && N * sizeof(double) <= (size_t)lds_max;
  const size_t fit = in_lds ? B : std::min(B, std::max<size_t>((size_t)e->roadmap_chunk_bytes / std::max<size_t>(N * sizeof(double), 1), 1));
  MJPL_TRY(e->d_rm_head.reserve(4, 64));
  size_t tmp_bytes = 0;
  MJPL_TRY(roadmap_space(st, B + 1, &tmp_bytes));
  RmQuery a = {};
  RmQuerySpans w = {};
  MJPL_TRY(carve_arena(e->d_rm_arena, [&](Carver &c) { carve_roadmap_query(c, B, C, emax, in_lds ? 0 : fit * N, np, tmp_bytes, &a, &w); }));
  HIP_TRY(hipMemsetAsync(dP, 0, B * (size_t)d.max_rows * np * sizeof(double), st));
  a.Q = dQ; a.row_off = drow_off; a.adj = dadj; a.w = dw;
  a.N = (int)N; a.d = (int)np; a.C = d.connections; a.max_rows = d.max_rows;
  a.QI = dQI; a.QG = dQG; a.B = (int)B;
  a.head = e->d_rm_head.p;
  a.P = dP; a.n_out = dn_out; a.status = dstatus; a.cost = dcost;
  PhaseLog phases;
  {
    PhaseScope ph(e, phases, 0);
    HIP_TRY(hipMemsetAsync(a.head, 0, 3 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_rm_finite, dim3(rm_grid(B)), dim3(kRmBlock), 0, st, dQI, dQG, (int)B, (int)np, w.cfg, w.fin);
    HIP_TRY(hipGetLastError());
    MJPL_TRY(launch_configs(e, w.cfg, (int64_t)(2 * B), MJPL_AOS, w.cvalid, nullptr));
    RmKnn q = {};
    q.X = w.cfg; q.xok = nullptr; q.M = (int)(2 * B); q.Q = dQ; q.qok = dnode_valid; q.N = (int)N; q.d = (int)np; q.k = d.connections;
    q.r2 = d.radius * d.radius; q.lo2 = 0.0; q.self = 0;
    q.nn_j = w.att_j; q.nn_d2 = w.att_d2; q.nn_cnt = w.att_cnt;
    MJPL_TRY(roadmap_knn(e, q));
    hipLaunchKernelGGL(k_rm_q_count, dim3(rm_grid(B + 1)), dim3(kRmBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (rocprim::exclusive_scan(w.tmp, tmp_bytes, a.cnt, a.off, 0, B + 1, rocprim::plus<int>(), st) != hipSuccess)
      return fail(MJPL_E_HIP, "rocprim::exclusive_scan failed");
    hipLaunchKernelGGL(k_rm_q_gather, dim3((unsigned)((B + kRmBlock / 64 - 1) / (kRmBlock / 64))), dim3(kRmBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
  }
  RoundHead h;
  MJPL_TRY(read_head(e, a.head, &h));
  const int64_t E = h.edges;
  e->roadmap_last_edges = E;
  if (E > 0) {
    PhaseScope ph(e, phases, 1);
    MJPL_TRY(launch_edges(e, a.QA, a.QB, E, d.step_dist, MJPL_AOS, 0, w.evalid, nullptr, few_long_edges(E, h.longest, d.step_dist)));
  }
  // (a large graph: more waves per problem hide the adjacency's latency; a small one: more problems per CU)
  const unsigned block = N >= 4096 ? 1024 : kRmBlock;
  const size_t lds = in_lds ? std::max<size_t>(N * sizeof(double), 8) : 0;
  if (lds > ((size_t)64 << 10))
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rm_search<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (size_t b0 = 0; b0 < B; b0 += fit) {
    a.b0 = (int)b0; a.nb = (int)std::min(fit, B - b0);
    PhaseScope ph(e, phases, 2);
    if (in_lds) hipLaunchKernelGGL(k_rm_search<true>, dim3((unsigned)a.nb), dim3(block), lds, st, a);
    else hipLaunchKernelGGL(k_rm_search<false>, dim3((unsigned)a.nb), dim3(block), 0, st, a);
    HIP_TRY(hipGetLastError());
    e->roadmap_last_chunks++;
  }
  // (the header once more, for the searches' sweeps.  Not read_head: that synchronises right after its copy, and here the
  //  status word's reset goes between the copy and the one synchronisation both wait for)
  unsigned long long head[3] = {0, 0, 0};
  HIP_TRY(hipMemcpyAsync(head, a.head, sizeof(head), hipMemcpyDeviceToHost, st));
  // an edge the edge kernels refuse counts as invalid here: the pipeline's status word is not this call's to report
  HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), st));
  HIP_TRY(hipStreamSynchronize(st));
  e->roadmap_last_sweeps = decode_head(head).live;
  return phase_sums(e, phases, e->roadmap_last_ms);
}

}  // namespace

// ---- certified edge checks (mjpl_sweep.h)
namespace {

int check_bounds(const mjpl_engine *e, const double *lo, const double *hi) {
  for (size_t k = 0; k < e->qidx.size(); k++) {
    const double l = lo ? lo[k] : -INFINITY, h = hi ? hi[k] : INFINITY;
    if (!(l <= h)) return fail(MJPL_E_ARG, "bounds of planning column %d: lo %g, hi %g (NaN and lo > hi are refused)", (int)k, l, h);
  }
  return MJPL_OK;
}

// the lever table for these bounds, made again only when they differ from those in force
int sweep_use_bounds(mjpl_engine *e, const double *lo, const double *hi) {
  bool same = e->d_sweep_tab != nullptr || e->qidx.empty();
  for (size_t k = 0; k < e->qidx.size() && same; k++)
    same = (lo ? lo[k] : -INFINITY) == e->sweep_lo[k] && (hi ? hi[k] : INFINITY) == e->sweep_hi[k];
  if (same) return MJPL_OK;
  HIP_TRY(hipStreamSynchronize(e->stream));
  return make_sweep_table(e, lo, hi);
}

int check_measure_args(const mjpl_engine *e, const void *Q, const void *HD, int64_t N, int layout, double cap,
                       std::initializer_list<const void *> outs) {
  MJPL_TRY(check_query_args(e, Q, N, layout, cap, outs));
  if (N > 0 && !HD) return fail(MJPL_E_ARG, "NULL batch pointer");
  if (!(cap < INFINITY)) return fail(MJPL_E_ARG, "cap must be finite, got %g", cap);
  return MJPL_OK;
}

// The descriptor of mjpl_sweep_edges* and mjpl_sweep_splines*: its ranges (NaN refused everywhere), lo <= hi per column
int check_sweep_desc(const mjpl_engine *e, const mjpl_sweep_desc *d) {
  if (!d) return fail(MJPL_E_ARG, "mjpl_sweep_edges: NULL descriptor");
  if (!(d->d_min >= 0) || !(d->d_min < INFINITY)) return fail(MJPL_E_ARG, "d_min must be >= 0 and finite (NaN is refused), got %g", d->d_min);
  if (!(d->cap > d->d_min + e->ct_margin_max) || !(d->cap < INFINITY))
    return fail(MJPL_E_ARG, "cap must be finite and > d_min + the largest margin of a non-allowed pair = %g (NaN is refused), got %g",
                d->d_min + e->ct_margin_max, d->cap);
  if (d->max_depth < 0 || d->max_depth > kSweepMaxDepth) return fail(MJPL_E_ARG, "max_depth must be 0..%d, got %d", kSweepMaxDepth, d->max_depth);
  return check_bounds(e, d->lo, d->hi);
}

// Argument checks of mjpl_sweep_edges*: check_common on both ends, the descriptor, every output non-null when E > 0.
int check_sweep_args(const mjpl_engine *e, const mjpl_sweep_desc *d, const void *QA, const void *QB, int64_t E, int layout,
                     std::initializer_list<const void *> outs) {
  MJPL_TRY(check_common(e, QA, E, layout));
  MJPL_TRY(check_common(e, QB, E, layout));
  MJPL_TRY(check_sweep_desc(e, d));
  if (E > 0)
    for (const void *o : outs)
      if (!o) return fail(MJPL_E_ARG, "NULL output pointer");
  return MJPL_OK;
}

// Argument checks of mjpl_sweep_splines*: the descriptor as for the edges, the offsets as for mjpl_topp_profile, W and
// every listed output non-null when B > 0.
int check_spline_sweep_args(const mjpl_engine *e, const mjpl_sweep_desc *d, const void *W, const int64_t *wp_off, int64_t B,
                            std::initializer_list<const void *> outs) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  if (B < 0 || B > INT32_MAX) return fail(MJPL_E_ARG, "mjpl_sweep_splines: batch size %lld out of range", (long long)B);
  MJPL_TRY(check_sweep_desc(e, d));
  if (B == 0) return MJPL_OK;
  if (!wp_off) return fail(MJPL_E_ARG, "mjpl_sweep_splines: NULL offsets");
  if (wp_off[0] != 0) return fail(MJPL_E_ARG, "wp_off[0] must be 0, got %lld", (long long)wp_off[0]);
  for (int64_t b = 0; b < B; b++) {
    const int64_t n = wp_off[b + 1] - wp_off[b];
    if (n < 2) return fail(MJPL_E_ARG, "path %lld has %lld waypoints (offsets must rise by at least 2)", (long long)b, (long long)n);
  }
  if (!W) return fail(MJPL_E_ARG, "NULL batch pointer");
  for (const void *o : outs)
    if (!o) return fail(MJPL_E_ARG, "NULL output pointer");
  return MJPL_OK;
}

// The loop of mjpl_sweep_edges* on device pointers (include/mjpl_hip.h states the node rule).  Edges go in chunks of
// clamp(kSweepNodes >> max_depth, 64, 2^14), so that a chunk's deepest round holds kSweepNodes nodes at most.  Per chunk:
// k_sweep_init writes round 0 into work buffer 0; then per round one k_distance<DM_SWEEP> launch over the open nodes, one
// k_sweep_step launch, and one 4-byte read of the other buffer's fill counter, which sizes the next round (0: the chunk
// is done); k_sweep_finish turns the per-edge state into the verdicts.  With `sp` the E "edges" are the pieces of a call's
// splines (launch_sweep_splines): the same loop, with the round-0 and step kernels of the cubic nodes.
int launch_sweep(mjpl_engine *e, const mjpl_sweep_desc &d, const double *dQA, const double *dQB, int64_t E, int layout,
                 int32_t *dstatus, double *dt_hit, double *dclear_lb, int32_t *dpair, int32_t *dnodes, int32_t *ddepth,
                 const SweepSpline *sp = nullptr) {
  MJPL_TRY(check_pair_types(e));
  MJPL_TRY(sweep_use_bounds(e, d.lo, d.hi));
  const int nplan = (int)e->qidx.size();
  const hipStream_t st = e->stream;
  if (!e->h_push_n) HIP_TRY(hipHostMalloc((void **)&e->h_push_n, sizeof(int)));
  const int64_t chunk = std::min<int64_t>(std::max<int64_t>(kSweepNodes >> d.max_depth, 64), (int64_t)1 << 14);
  const size_t np = (size_t)std::max(nplan, 1);
  // a work buffer for n nodes; its fill counter sits behind the (edge, ordinal) words
  auto reserve_work = [&](int k, size_t n) -> int {
    MJPL_TRY(e->d_sweep_rows[k].reserve(n * np));
    MJPL_TRY(e->d_sweep_hd[k].reserve(n * np));
    return e->d_sweep_meta[k].reserve(2 * n + 1);
  };
  auto work = [&](int k) {
    return SweepWork{e->d_sweep_rows[k].p, e->d_sweep_hd[k].p, e->d_sweep_meta[k].p, e->d_sweep_meta[k].p + e->d_sweep_meta[k].cap - 1};
  };
  auto read_count = [&](const SweepWork &w, int *n) -> int {
    HIP_TRY(hipMemcpyAsync(e->h_push_n, w.n, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *n = *e->h_push_n;
    return MJPL_OK;
  };
  MJPL_TRY(e->d_sweep_key.reserve((size_t)std::min<int64_t>(chunk, E)));
  SweepArgs a = {};
  a.QA = dQA; a.QB = dQB; a.E = E; a.layout = layout; a.nplan = nplan;
  a.lo = e->d_sweep_tab; a.hi = e->d_sweep_tab + nplan;
  a.d_min = d.d_min; a.max_depth = d.max_depth;
  a.key = e->d_sweep_key.p;
  a.status = dstatus; a.nodes = dnodes; a.depth = ddepth; a.pair = dpair; a.t_hit = dt_hit;
  a.clear_bits = reinterpret_cast<unsigned long long *>(dclear_lb);
  for (int64_t i0 = 0; i0 < E; i0 += chunk) {
    const int ne = (int)std::min<int64_t>(chunk, E - i0);
    a.i0 = i0;
    MJPL_TRY(reserve_work(0, 3 * (size_t)ne));
    SweepWork cur = work(0);
    HIP_TRY(hipMemsetAsync(cur.n, 0, sizeof(int), st));
    const dim3 init_grid((unsigned)((ne + kSweepBlock - 1) / kSweepBlock));
    if (sp) hipLaunchKernelGGL(k_sweep_spline_init, init_grid, dim3(kSweepBlock), 0, st, a, *sp, ne, cur);
    else hipLaunchKernelGGL(k_sweep_init, init_grid, dim3(kSweepBlock), 0, st, a, ne, cur);
    HIP_TRY(hipGetLastError());
    int n = 0;
    MJPL_TRY(read_count(cur, &n));
    for (int round = 0; round <= d.max_depth && n > 0; round++) {
      const int nxt = (round & 1) ^ 1;
      MJPL_TRY(e->d_sweep_f64.reserve(2 * (size_t)n));
      MJPL_TRY(e->d_sweep_i32.reserve(2 * (size_t)n));
      double *gap = e->d_sweep_f64.p, *slack = gap + n;
      int *gap_pair = e->d_sweep_i32.p, *slack_pair = gap_pair + n;
      MJPL_TRY(launch_distance(e, DM_SWEEP, cur.rows, n, MJPL_AOS, d.cap, nullptr, gap, gap_pair, nullptr, nullptr, nullptr,
                               nullptr, 0, nullptr, cur.hd, slack, slack_pair));
      // (the other buffer at twice the active count: every node may open two)
      const bool last = round == d.max_depth;
      MJPL_TRY(reserve_work(nxt, last ? 1 : 2 * (size_t)n));
      SweepWork next = work(nxt);
      HIP_TRY(hipMemsetAsync(next.n, 0, sizeof(int), st));
      const dim3 step_grid((unsigned)((n + kSweepBlock - 1) / kSweepBlock));
      if (sp) hipLaunchKernelGGL(k_sweep_spline_step, step_grid, dim3(kSweepBlock), 0, st, a, *sp, round, n, cur, gap, gap_pair, slack, next);
      else hipLaunchKernelGGL(k_sweep_step, step_grid, dim3(kSweepBlock), 0, st, a, round, n, cur, gap, gap_pair, slack, next);
      HIP_TRY(hipGetLastError());
      if (last) break;
      MJPL_TRY(read_count(next, &n));
      cur = next;
    }
    hipLaunchKernelGGL(k_sweep_finish, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, a, ne);
    HIP_TRY(hipGetLastError());
  }
  return MJPL_OK;
}

// mjpl_sweep_splines* on device batches (wp_off on the host).  The stream is drained, then the call's tables go up:
// wp_off for k_topp_spline and per piece the row of its first waypoint and n - 1.  k_topp_spline writes M (into the
// engine's own buffer when the caller wants none); launch_sweep runs the loop over the pieces.
int launch_sweep_splines(mjpl_engine *e, const mjpl_sweep_desc &d, const double *dW, const int64_t *wp_off, int64_t B, double *dM,
                         int32_t *dstatus, double *dt_hit, double *dclear_lb, int32_t *dpair, int32_t *dnodes, int32_t *ddepth) {
  const int nplan = (int)e->qidx.size();
  if (nplan < 1) return fail(MJPL_E_ARG, "mjpl_sweep_splines: no planning columns");
  HIP_TRY(hipStreamSynchronize(e->stream));
  const size_t nb = (size_t)B + 1, pieces = (size_t)(wp_off[B] - B);
  e->sweep_piece_h.resize(nb + 2 * pieces);
  std::copy(wp_off, wp_off + nb, e->sweep_piece_h.begin());
  int64_t *piece = e->sweep_piece_h.data() + nb;
  for (int64_t b = 0; b < B; b++)
    for (int64_t k = wp_off[b]; k < wp_off[b + 1] - 1; k++) {
      piece[2 * (k - b)] = k;
      piece[2 * (k - b) + 1] = wp_off[b + 1] - wp_off[b] - 1;
    }
  MJPL_TRY(e->d_sweep_piece.reserve(e->sweep_piece_h.size(), 1024));
  HIP_TRY(hipMemcpyAsync(e->d_sweep_piece.p, e->sweep_piece_h.data(), e->sweep_piece_h.size() * sizeof(int64_t),
                         hipMemcpyHostToDevice, e->stream));
  MJPL_TRY(topp_cp_table(e, wp_off, B));
  if (!dM) {
    MJPL_TRY(e->d_sweep_M.reserve((size_t)wp_off[B] * nplan));
    dM = e->d_sweep_M.p;
  }
  ToppBatch t = {};
  t.W = dW; t.wp_off = e->d_sweep_piece.p; t.B = (int)B; t.d = nplan; t.cp = e->d_topp_cp.p; t.M = dM;
  hipLaunchKernelGGL(k_topp_spline, dim3((unsigned)((B * nplan + 255) / 256)), dim3(256), 0, e->stream, t);
  HIP_TRY(hipGetLastError());
  const SweepSpline sp = {dW, dM, e->d_sweep_piece.p + nb};
  return launch_sweep(e, d, nullptr, nullptr, (int64_t)pieces, MJPL_AOS, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth, &sp);
}

}  // namespace

extern "C" {

int mjpl_nearest_dev(mjpl_engine *e, const double *dnodes, int64_t n, int64_t cap, const double *dqueries,
                     int64_t M, int32_t *dout_idx, double *dout_dist2) {
  if (!e || n < 0 || M < 0 || cap < n) return fail(MJPL_E_ARG, "mjpl_nearest_dev: bad sizes");
  if (M == 0) return MJPL_OK;
  if (!dnodes || !dqueries || !dout_idx) return fail(MJPL_E_ARG, "mjpl_nearest_dev: NULL pointer");
  return nearest_core(e, e->nn, {dnodes, n, cap, dqueries, M, dout_idx, dout_dist2, nullptr, e->stream});
}

int mjpl_nearest_range_dev(mjpl_engine *e, const double *dnodes, int64_t n0, int64_t n, int64_t cap, const double *dqueries,
                           int64_t M, int32_t *dout_idx, double *dout_dist2, const int32_t *dprev_idx, const double *dprev_dist2) {
  if (!e || n < 0 || n0 < 0 || n0 > n || M < 0 || cap < n) return fail(MJPL_E_ARG, "mjpl_nearest_range_dev: bad sizes");
  if (M == 0) return MJPL_OK;
  if (!dnodes || !dqueries || !dout_idx || ((dprev_idx == nullptr) != (dprev_dist2 == nullptr)))
    return fail(MJPL_E_ARG, "mjpl_nearest_range_dev: NULL pointer");
  return nearest_range(e, e->nn, e->stream, dnodes, n0, n, cap, dqueries, M, dout_idx, dout_dist2, dprev_idx, dprev_dist2);
}

// ---- host-buffer

int mjpl_check_configs(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, uint8_t *valid) {
  int rc = check_common(e, Q, N, layout);
  if (rc != MJPL_OK) return rc;
  if (N == 0) return MJPL_OK;
  if (!valid) return fail(MJPL_E_ARG, "NULL output pointer");
  const size_t qb = (size_t)N * e->qidx.size() * sizeof(double);
  return staged(e, true, {{Q, qb}}, {{valid, (size_t)N}}, [&](void **in, void **out) {
    return launch_configs(e, (const double *)in[0], N, layout, (uint8_t *)out[0], nullptr);
  });
}

int mjpl_check_edges(mjpl_engine *e, const double *QA, const double *QB, int64_t E, double step_dist,
                     int32_t layout, int32_t flags, uint8_t *valid, int32_t *first_bad) {
  int rc = check_common(e, QA, E, layout);
  if (rc != MJPL_OK) return rc;
  if (!(step_dist > 0.0)) return fail(MJPL_E_ARG, "`step_dist` must be > 0");
  if (E == 0) return MJPL_OK;
  if (!QB || !valid) return fail(MJPL_E_ARG, "NULL pointer");
  const size_t qb = (size_t)E * e->qidx.size() * sizeof(double);
  // (few_long_edges) The rows are in host memory here, so a small batch can simply be looked at.
  bool long_edges = false;
  if (E <= kFewEdges) {
    const int64_t np = (int64_t)e->qidx.size();
    double longest2 = 0;
    for (int64_t i = 0; i < E; i++) {
      double s = 0;
      for (int64_t k = 0; k < np; k++) {
        const double d = layout == MJPL_SOA ? QB[k * E + i] - QA[k * E + i] : QB[i * np + k] - QA[i * np + k];
        s += d * d;
      }
      if (s > longest2) longest2 = s;  // (a NaN never compares greater: such an edge is reported by the kernels)
    }
    long_edges = few_long_edges(E, std::sqrt(longest2), step_dist);
  }
  int status = 0;
  const HostOut outs[] = {{valid, (size_t)E}, {first_bad, (size_t)E * sizeof(int32_t)}, {&status, sizeof(int), e->d_status}};
  rc = staged(e, true, {{QA, qb}, {QB, qb}}, outs, [&](void **in, void **out) {
    HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), e->stream));
    return launch_edges(e, (const double *)in[0], (const double *)in[1], E, step_dist, layout, flags, (uint8_t *)out[0],
                        (int32_t *)out[1], long_edges);
  });
  return rc != MJPL_OK ? rc : edge_status(status);
}

int mjpl_fk(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double *xpos, double *xquat,
            double *geom_xpos, double *geom_xmat) {
  int rc = check_common(e, Q, N, layout);
  if (rc != MJPL_OK) return rc;
  if (N == 0) return MJPL_OK;
  const HostModel &m = e->m;
  const size_t n = (size_t)N, qb = n * e->qidx.size() * sizeof(double);
  const HostOut outs[] = {{xpos, n * m.nbody * 3 * 8}, {xquat, n * m.nbody * 4 * 8}, {geom_xpos, n * m.ngeom * 3 * 8},
                          {geom_xmat, n * m.ngeom * 9 * 8}};
  rc = staged(e, false, {{Q, qb}}, outs, [&](void **in, void **out) {
    FkOut fo;
    fo.xpos = (double *)out[0];
    fo.xquat = (double *)out[1];
    fo.geom_xpos = (double *)out[2];
    fo.geom_xmat = (double *)out[3];
    fo.nbody = m.nbody;
    fo.ngeom = m.ngeom;
    const size_t lds = lds_bytes(e, 1);
    const int rc2 = allow_lds(k_fk, lds);
    if (rc2 != MJPL_OK) return rc2;
    hipLaunchKernelGGL(k_fk, dim3((unsigned)((N + kBlock - 1) / kBlock)), dim3(kBlock), lds, e->stream, e->d_ip,
                       (int)e->ip.size(), e->d_dp, (int)e->dp.size(), (const double *)in[0], N, layout, fo);
    HIP_TRY(hipGetLastError());
    return MJPL_OK;
  });
  if (rc != MJPL_OK) return rc;
  // bodies/geoms welded to the world do not depend on qpos: poses folded at create
  for (int64_t i = 0; i < N; i++) {
    for (int b = 0; b < m.nbody; b++) {
      if (!e->lay.body_static[b]) continue;
      if (xpos) memcpy(xpos + (i * m.nbody + b) * 3, &e->lay.st_xpos[3 * b], 3 * sizeof(double));
      if (xquat) memcpy(xquat + (i * m.nbody + b) * 4, &e->lay.st_xquat[4 * b], 4 * sizeof(double));
    }
    for (int g = 0; g < m.ngeom; g++) {
      if (!e->lay.geom_static[g]) continue;
      if (geom_xpos) memcpy(geom_xpos + (i * m.ngeom + g) * 3, &e->lay.st_gxpos[3 * g], 3 * sizeof(double));
      if (geom_xmat) memcpy(geom_xmat + (i * m.ngeom + g) * 9, &e->lay.st_gxmat[9 * g], 9 * sizeof(double));
    }
  }
  return MJPL_OK;
}

// ---- contacts: which candidate pairs touch (mjpl_contacts.h)

int32_t mjpl_contact_pair_count(mjpl_engine *e) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  return (int32_t)e->ct_g1.size();
}

int mjpl_contact_pairs(mjpl_engine *e, int32_t *geom1, int32_t *geom2, uint8_t *allowed, int32_t cap) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  const int32_t P = (int32_t)e->ct_g1.size();
  if (cap < P) return fail(MJPL_E_ARG, "mjpl_contact_pairs: cap %d < %d candidate pairs", cap, P);
  if (P > 0 && (!geom1 || !geom2 || !allowed)) return fail(MJPL_E_ARG, "mjpl_contact_pairs: NULL output pointer");
  for (int32_t p = 0; p < P; p++) {
    geom1[p] = e->ct_g1[p];
    geom2[p] = e->ct_g2[p];
    allowed[p] = e->ct_allowed[p];
  }
  return MJPL_OK;
}

int mjpl_contacts_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, uint64_t *dbits) {
  int rc = check_query_args(e, dQ, N, layout, INFINITY, {});
  if (rc != MJPL_OK) return rc;
  if (N > 0 && !e->ct_g1.empty() && !dbits) return fail(MJPL_E_ARG, "NULL output pointer");
  HIP_TRY(hipSetDevice(e->device));
  return launch_contacts(e, dQ, N, layout, reinterpret_cast<unsigned long long *>(dbits));
}

int mjpl_contacts(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, uint64_t *bits) {
  int rc = check_query_args(e, Q, N, layout, INFINITY, {});
  if (rc != MJPL_OK) return rc;
  const int64_t W = ((int64_t)e->ct_g1.size() + 63) / 64;
  if (N == 0 || W == 0) return MJPL_OK;
  if (!bits) return fail(MJPL_E_ARG, "NULL output pointer");
  const size_t qb = (size_t)N * e->qidx.size() * sizeof(double);
  return staged(e, false, {{Q, qb}}, {{bits, (size_t)N * (size_t)W * sizeof(uint64_t)}}, [&](void **in, void **out) {
    return launch_contacts(e, (const double *)in[0], N, layout, (unsigned long long *)out[0]);
  });
}

// ---- distances and clearance per configuration (mjpl_distance.h)

int mjpl_distances_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax, double *ddist) {
  int rc = check_query_args(e, dQ, N, layout, distmax, {ddist});
  if (rc != MJPL_OK) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_distance(e, DM_DIST, dQ, N, layout, distmax, ddist, nullptr, nullptr);
}

int mjpl_distances(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax, double *dist) {
  int rc = check_query_args(e, Q, N, layout, distmax, {dist});
  if (rc != MJPL_OK) return rc;
  const size_t P = e->ct_g1.size();
  if (N == 0 || P == 0) return MJPL_OK;
  const size_t qb = (size_t)N * e->qidx.size() * sizeof(double);
  return staged(e, false, {{Q, qb}}, {{dist, (size_t)N * P * sizeof(double)}}, [&](void **in, void **out) {
    return launch_distance(e, DM_DIST, (const double *)in[0], N, layout, distmax, (double *)out[0], nullptr, nullptr);
  });
}

int mjpl_clearance_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax, double *dclear,
                       int32_t *dpair) {
  int rc = check_query_args(e, dQ, N, layout, distmax, {dclear, dpair});
  if (rc != MJPL_OK || N == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_distance(e, DM_CLEAR, dQ, N, layout, distmax, nullptr, dclear, dpair);
}

int mjpl_clearance(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax, double *clear,
                   int32_t *pair) {
  int rc = check_query_args(e, Q, N, layout, distmax, {clear, pair});
  if (rc != MJPL_OK || N == 0) return rc;
  const size_t n = N, qb = n * e->qidx.size() * sizeof(double);
  return staged(e, false, {{Q, qb}}, {{clear, n * sizeof(double)}, {pair, n * sizeof(int32_t)}}, [&](void **in, void **out) {
    return launch_distance(e, DM_CLEAR, (const double *)in[0], N, layout, distmax, nullptr, (double *)out[0], (int32_t *)out[1]);
  });
}

// ---- clearance gradients and witness points per configuration (mjpl_distance_grad.h)

int mjpl_clearance_grad_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax, double *dclear,
                            int32_t *dpair, double *dgrad, double *dfromto, double *dnormal, int32_t *dstatus) {
  int rc = check_query_args(e, dQ, N, layout, distmax, {dclear, dpair, dgrad, dstatus});
  if (rc != MJPL_OK || N == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_distance(e, DM_GRAD, dQ, N, layout, distmax, nullptr, dclear, dpair, dgrad, dfromto, dnormal, dstatus);
}

int mjpl_clearance_grad(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax, double *clear,
                        int32_t *pair, double *grad, double *fromto, double *normal, int32_t *status) {
  int rc = check_query_args(e, Q, N, layout, distmax, {clear, pair, grad, status});
  if (rc != MJPL_OK || N == 0) return rc;
  const size_t n = N, db = sizeof(double), ib = sizeof(int32_t), qb = n * e->qidx.size() * db;
  const HostOut outs[] = {{clear, n * db}, {pair, n * ib}, {grad, qb}, {fromto, n * 6 * db}, {normal, n * 3 * db}, {status, n * ib}};
  return staged(e, false, {{Q, qb}}, outs, [&](void **in, void **out) {
    return launch_distance(e, DM_GRAD, (const double *)in[0], N, layout, distmax, nullptr, (double *)out[0], (int32_t *)out[1],
                           (double *)out[2], (double *)out[3], (double *)out[4], (int32_t *)out[5]);
  });
}

// ---- every pair within distmax: distance, witnesses and gradient (mjpl_distance_grad.h: near_step)

int mjpl_near_pairs_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, double distmax, int32_t K,
                        int32_t *dcount, int32_t *dpair, double *ddist, double *dgrad, double *dfromto, double *dnormal,
                        int32_t *dstatus) {
  int rc = check_query_args(e, dQ, N, layout, distmax, {dcount, dpair, ddist, dgrad, dstatus});
  if (rc == MJPL_OK && K < 1) rc = fail(MJPL_E_ARG, "K must be >= 1, got %d", K);
  if (rc != MJPL_OK || N == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_distance(e, DM_NEAR, dQ, N, layout, distmax, ddist, nullptr, dpair, dgrad, dfromto, dnormal, dstatus, K,
                         dcount);
}

int mjpl_near_pairs(mjpl_engine *e, const double *Q, int64_t N, int32_t layout, double distmax, int32_t K, int32_t *count,
                    int32_t *pair, double *dist, double *grad, double *fromto, double *normal, int32_t *status) {
  int rc = check_query_args(e, Q, N, layout, distmax, {count, pair, dist, grad, status});
  if (rc == MJPL_OK && K < 1) rc = fail(MJPL_E_ARG, "K must be >= 1, got %d", K);
  if (rc != MJPL_OK || N == 0) return rc;
  const size_t n = N, nk = n * (size_t)K, db = sizeof(double), ib = sizeof(int32_t), np = e->qidx.size();
  // (all but count and pair are written in the listed slots only: the caller's other bytes are kept)
  const HostOut outs[] = {{count, n * ib},           {pair, nk * ib},           {dist, nk * db, nullptr, true},
                          {grad, nk * np * db, nullptr, true}, {fromto, nk * 6 * db, nullptr, true},
                          {normal, nk * 3 * db, nullptr, true}, {status, nk * ib, nullptr, true}};
  return staged(e, false, {{Q, n * np * db}}, outs, [&](void **in, void **out) {
    return launch_distance(e, DM_NEAR, (const double *)in[0], N, layout, distmax, (double *)out[2], nullptr,
                           (int32_t *)out[1], (double *)out[3], (double *)out[4], (double *)out[5], (int32_t *)out[6], K,
                           (int32_t *)out[0]);
  });
}

// ---- push out to a minimum clearance (mjpl_push.h)

int mjpl_push_out_dev(mjpl_engine *e, const mjpl_push_desc *d, const double *dQ, int64_t N, int32_t layout, double *dQ_out,
                      double *dclear, int32_t *dpair, int32_t *diters, int32_t *dstatus) {
  int rc = check_push_args(e, d, dQ, N, layout, {dQ_out, dclear, dpair, diters, dstatus});
  if (rc != MJPL_OK || N == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_push(e, *d, dQ, N, layout, dQ_out, dclear, dpair, diters, dstatus);
}

int mjpl_push_out(mjpl_engine *e, const mjpl_push_desc *d, const double *Q, int64_t N, int32_t layout, double *Q_out,
                  double *clear, int32_t *pair, int32_t *iters, int32_t *status) {
  int rc = check_push_args(e, d, Q, N, layout, {Q_out, clear, pair, iters, status});
  if (rc != MJPL_OK || N == 0) return rc;
  const size_t n = N, db = sizeof(double), ib = sizeof(int32_t), qb = n * e->qidx.size() * db;
  const HostOut outs[] = {{Q_out, qb}, {clear, n * db}, {pair, n * ib}, {iters, n * ib}, {status, n * ib}};
  return staged(e, false, {{Q, qb}}, outs, [&](void **in, void **out) {
    return launch_push(e, *d, (const double *)in[0], N, layout, (double *)out[0], (double *)out[1], (int32_t *)out[2],
                       (int32_t *)out[3], (int32_t *)out[4]);
  });
}

// ---- time-optimal path parameterisation (mjpl_topp.h)

int mjpl_topp_profile_dev(mjpl_engine *e, const mjpl_topp_desc *d, const double *dW, const int64_t *wp_off, int64_t B, double *dM,
                          double *dx, double *du, double *dt, int32_t *dstatus) {
  int rc = check_topp_args(e, d, dW, wp_off, B, {dM, dx, du, dt, dstatus});
  if (rc == MJPL_OK && B == 0) e->topp_last_chunks = 0;
  if (rc != MJPL_OK || B == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_topp_profile(e, *d, dW, wp_off, B, dM, dx, du, dt, dstatus);
}

int mjpl_topp_profile(mjpl_engine *e, const mjpl_topp_desc *d, const double *W, const int64_t *wp_off, int64_t B, double *M,
                      double *x, double *u, double *t, int32_t *status) {
  int rc = check_topp_args(e, d, W, wp_off, B, {M, x, u, t, status});
  if (rc == MJPL_OK && B == 0) e->topp_last_chunks = 0;
  if (rc != MJPL_OK || B == 0) return rc;
  const size_t db = sizeof(double), wb = (size_t)wp_off[B] * d->nq * db, gb = (size_t)topp_g_off_h(wp_off, d->grid, B) * db;
  const HostOut outs[] = {{M, wb}, {x, gb}, {u, gb}, {t, gb}, {status, (size_t)B * sizeof(int32_t)}};
  return staged(e, false, {{W, wb}}, outs, [&](void **in, void **out) {
    return launch_topp_profile(e, *d, (const double *)in[0], wp_off, B, (double *)out[0], (double *)out[1], (double *)out[2],
                               (double *)out[3], (int32_t *)out[4]);
  });
}

int mjpl_topp_sample_dev(mjpl_engine *e, const mjpl_topp_desc *d, const double *dW, const int64_t *wp_off, int64_t B,
                         const double *dM, const double *dx, const double *du, const double *dt_grid, double dt,
                         const int64_t *samp_off, double *dpos, double *dvel, double *dacc) {
  int rc = check_topp_args(e, d, dW, wp_off, B, {dM, dx, du, dt_grid});
  if (rc == MJPL_OK) rc = check_topp_sample_args(wp_off, B, dt, samp_off);
  if (rc != MJPL_OK || B == 0 || samp_off[B] == 0) return rc;
  if (!dpos || !dvel || !dacc) return fail(MJPL_E_ARG, "NULL output pointer");
  HIP_TRY(hipSetDevice(e->device));
  return launch_topp_sample(e, *d, dW, wp_off, B, dM, dx, du, dt_grid, dt, samp_off, dpos, dvel, dacc);
}

int mjpl_topp_sample(mjpl_engine *e, const mjpl_topp_desc *d, const double *W, const int64_t *wp_off, int64_t B, const double *M,
                     const double *x, const double *u, const double *t, double dt, const int64_t *samp_off, double *pos,
                     double *vel, double *acc) {
  int rc = check_topp_args(e, d, W, wp_off, B, {M, x, u, t});
  if (rc == MJPL_OK) rc = check_topp_sample_args(wp_off, B, dt, samp_off);
  if (rc != MJPL_OK || B == 0 || samp_off[B] == 0) return rc;
  if (!pos || !vel || !acc) return fail(MJPL_E_ARG, "NULL output pointer");
  const size_t db = sizeof(double), wb = (size_t)wp_off[B] * d->nq * db, gb = (size_t)topp_g_off_h(wp_off, d->grid, B) * db;
  const size_t sb = (size_t)samp_off[B] * d->nq * db;
  return staged(e, false, {{W, wb}, {M, wb}, {x, gb}, {u, gb}, {t, gb}}, {{pos, sb}, {vel, sb}, {acc, sb}}, [&](void **in, void **out) {
    return launch_topp_sample(e, *d, (const double *)in[0], wp_off, B, (const double *)in[1], (const double *)in[2],
                              (const double *)in[3], (const double *)in[4], dt, samp_off, (double *)out[0], (double *)out[1],
                              (double *)out[2]);
  });
}

// ---- jerk-limited path parameterisation (mjpl_jerk.h)

int mjpl_jerk_profile_dev(mjpl_engine *e, const mjpl_jerk_desc *d, const double *dW, const int64_t *wp_off, int64_t B, double *dM,
                          double *dlim, double *dv, double *dvp, double *dtc, double *dt, int32_t *dstatus) {
  int rc = check_jerk_args(e, d, dW, wp_off, B, {dM, dlim, dv, dvp, dtc, dt, dstatus});
  if (rc != MJPL_OK || B == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_jerk_profile(e, *d, dW, wp_off, B, dM, dlim, dv, dvp, dtc, dt, dstatus);
}

int mjpl_jerk_profile(mjpl_engine *e, const mjpl_jerk_desc *d, const double *W, const int64_t *wp_off, int64_t B, double *M,
                      double *lim, double *v, double *vp, double *tc, double *t, int32_t *status) {
  int rc = check_jerk_args(e, d, W, wp_off, B, {M, lim, v, vp, tc, t, status});
  if (rc != MJPL_OK || B == 0) return rc;
  const size_t db = sizeof(double), wb = (size_t)wp_off[B] * d->nq * db, gb = (size_t)topp_g_off_h(wp_off, d->grid, B) * db;
  const HostOut outs[] = {{M, wb}, {lim, 3 * gb}, {v, gb}, {vp, gb}, {tc, gb}, {t, gb}, {status, (size_t)B * sizeof(int32_t)}};
  return staged(e, false, {{W, wb}}, outs, [&](void **in, void **out) {
    return launch_jerk_profile(e, *d, (const double *)in[0], wp_off, B, (double *)out[0], (double *)out[1], (double *)out[2],
                               (double *)out[3], (double *)out[4], (double *)out[5], (int32_t *)out[6]);
  });
}

int mjpl_jerk_sample_dev(mjpl_engine *e, const mjpl_jerk_desc *d, const double *dW, const int64_t *wp_off, int64_t B,
                         const double *dM, const double *dlim, const double *dv, const double *dvp, const double *dtc,
                         const double *dt_grid, double dt, const int64_t *samp_off, double *dpos, double *dvel, double *dacc) {
  int rc = check_jerk_args(e, d, dW, wp_off, B, {dM, dlim, dv, dvp, dtc, dt_grid});
  if (rc == MJPL_OK) rc = check_topp_sample_args(wp_off, B, dt, samp_off);
  if (rc != MJPL_OK || B == 0 || samp_off[B] == 0) return rc;
  if (!dpos || !dvel || !dacc) return fail(MJPL_E_ARG, "NULL output pointer");
  HIP_TRY(hipSetDevice(e->device));
  return launch_jerk_sample(e, *d, dW, wp_off, B, dM, dlim, dv, dvp, dtc, dt_grid, dt, samp_off, dpos, dvel, dacc);
}

int mjpl_jerk_sample(mjpl_engine *e, const mjpl_jerk_desc *d, const double *W, const int64_t *wp_off, int64_t B, const double *M,
                     const double *lim, const double *v, const double *vp, const double *tc, const double *t, double dt,
                     const int64_t *samp_off, double *pos, double *vel, double *acc) {
  int rc = check_jerk_args(e, d, W, wp_off, B, {M, lim, v, vp, tc, t});
  if (rc == MJPL_OK) rc = check_topp_sample_args(wp_off, B, dt, samp_off);
  if (rc != MJPL_OK || B == 0 || samp_off[B] == 0) return rc;
  if (!pos || !vel || !acc) return fail(MJPL_E_ARG, "NULL output pointer");
  const size_t db = sizeof(double), wb = (size_t)wp_off[B] * d->nq * db, gb = (size_t)topp_g_off_h(wp_off, d->grid, B) * db;
  const size_t sb = (size_t)samp_off[B] * d->nq * db;
  return staged(e, false, {{W, wb}, {M, wb}, {lim, 3 * gb}, {v, gb}, {vp, gb}, {tc, gb}, {t, gb}}, {{pos, sb}, {vel, sb}, {acc, sb}},
                [&](void **in, void **out) {
    return launch_jerk_sample(e, *d, (const double *)in[0], wp_off, B, (const double *)in[1], (const double *)in[2],
                              (const double *)in[3], (const double *)in[4], (const double *)in[5], (const double *)in[6], dt,
                              samp_off, (double *)out[0], (double *)out[1], (double *)out[2]);
  });
}

// ---- path shortcutting (mjpl_shortcut.h)

int mjpl_shortcut_paths_dev(mjpl_engine *e, const mjpl_shortcut_desc *d, const double *dW, const int64_t *wp_off, int64_t B,
                            uint8_t *dkeep, int32_t *dn_out, double *dlength, int32_t *dstatus, int32_t *dproposed,
                            int32_t *daccepted) {
  int rc = check_shortcut_args(e, d, dW, wp_off, B, dkeep, dn_out, dstatus);
  if (rc == MJPL_OK && B == 0) shortcut_reset(e);
  if (rc != MJPL_OK || B == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_shortcut(e, *d, dW, wp_off, B, dkeep, dn_out, dlength, dstatus, dproposed, daccepted);
}

int mjpl_shortcut_paths(mjpl_engine *e, const mjpl_shortcut_desc *d, const double *W, const int64_t *wp_off, int64_t B, uint8_t *keep,
                        int32_t *n_out, double *length, int32_t *status, int32_t *proposed, int32_t *accepted) {
  int rc = check_shortcut_args(e, d, W, wp_off, B, keep, n_out, status);
  if (rc == MJPL_OK && B == 0) shortcut_reset(e);
  if (rc != MJPL_OK || B == 0) return rc;
  const size_t wb = (size_t)wp_off[B] * e->qidx.size() * sizeof(double), ib = (size_t)B * sizeof(int32_t);
  const HostOut outs[] = {{keep, (size_t)wp_off[B]}, {n_out, ib}, {length, (size_t)B * sizeof(double)}, {status, ib}, {proposed, ib},
                          {accepted, ib}};
  return staged(e, false, {{W, wb}}, outs, [&](void **in, void **out) {
    return launch_shortcut(e, *d, (const double *)in[0], wp_off, B, (uint8_t *)out[0], (int32_t *)out[1], (double *)out[2],
                           (int32_t *)out[3], (int32_t *)out[4], (int32_t *)out[5]);
  });
}

// ---- planning in lockstep (mjpl_plan.h)

int mjpl_plan_paths_dev(mjpl_engine *e, const mjpl_plan_desc *d, const double *dQI, const double *dQG, int64_t B, const double *lo,
                        const double *hi, double *dP, int32_t *dn_out, int32_t *dstatus, int32_t *drounds_used, int32_t *dedges,
                        int32_t *dtree_nodes) {
  int rc = check_plan_args(e, d, dQI, dQG, B, lo, hi, dP, dn_out, dstatus);
  if (rc == MJPL_OK && B == 0) plan_reset(e);
  if (rc != MJPL_OK || B == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_plan(e, *d, dQI, dQG, B, lo, hi, dP, dn_out, dstatus, drounds_used, dedges, dtree_nodes);
}

int mjpl_plan_paths(mjpl_engine *e, const mjpl_plan_desc *d, const double *QI, const double *QG, int64_t B, const double *lo,
                    const double *hi, double *P, int32_t *n_out, int32_t *status, int32_t *rounds_used, int32_t *edges,
                    int32_t *tree_nodes) {
  int rc = check_plan_args(e, d, QI, QG, B, lo, hi, P, n_out, status);
  if (rc == MJPL_OK && B == 0) plan_reset(e);
  if (rc != MJPL_OK || B == 0) return rc;
  const size_t qb = (size_t)B * e->qidx.size() * sizeof(double), ib = (size_t)B * sizeof(int32_t);
  const HostOut outs[] = {{P, qb * ((size_t)d->rounds + 2)}, {n_out, ib}, {status, ib}, {rounds_used, ib}, {edges, ib}, {tree_nodes, 2 * ib}};
  return staged(e, false, {{QI, qb}, {QG, qb}}, outs, [&](void **in, void **out) {
    return launch_plan(e, *d, (const double *)in[0], (const double *)in[1], B, lo, hi, (double *)out[0], (int32_t *)out[1],
                       (int32_t *)out[2], (int32_t *)out[3], (int32_t *)out[4], (int32_t *)out[5]);
  });
}

// ---- roadmap planning (mjpl_roadmap.h)

int mjpl_roadmap_build_dev(mjpl_engine *e, const mjpl_roadmap_desc *d, const double *dQ, int64_t N, uint8_t *dnode_valid, int32_t *drow_off,
                           int32_t *dadj, double *dw) {
  int rc = check_roadmap_build_args(e, d, dQ, N, dnode_valid, drow_off, dadj, dw);
  if (rc == MJPL_OK && N == 0) roadmap_reset(e);
  if (rc != MJPL_OK || N == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_roadmap_build(e, *d, dQ, N, dnode_valid, drow_off, dadj, dw);
}

int mjpl_roadmap_build(mjpl_engine *e, const mjpl_roadmap_desc *d, const double *Q, int64_t N, uint8_t *node_valid, int32_t *row_off,
                       int32_t *adj, double *w) {
  int rc = check_roadmap_build_args(e, d, Q, N, node_valid, row_off, adj, w);
  if (rc == MJPL_OK && N == 0) roadmap_reset(e);
  if (rc != MJPL_OK || N == 0) return rc;
  const size_t n = (size_t)N, cap = 2 * n * (size_t)d->k;
  const HostOut outs[] = {{node_valid, n}, {row_off, (n + 1) * sizeof(int32_t)}, {adj, cap * sizeof(int32_t)}, {w, cap * sizeof(double)}};
  return staged(e, false, {{Q, n * e->qidx.size() * sizeof(double)}}, outs, [&](void **in, void **out) {
    return launch_roadmap_build(e, *d, (const double *)in[0], N, (uint8_t *)out[0], (int32_t *)out[1], (int32_t *)out[2], (double *)out[3]);
  });
}

int mjpl_roadmap_query_dev(mjpl_engine *e, const mjpl_roadmap_query_desc *d, const double *dQ, int64_t N, const uint8_t *dnode_valid,
                           const int32_t *drow_off, const int32_t *dadj, const double *dw, const double *dQI, const double *dQG, int64_t B,
                           double *dP, int32_t *dn_out, int32_t *dstatus, double *dcost) {
  int rc = check_roadmap_query_args(e, d, dQ, N, dnode_valid, drow_off, dadj, dw, dQI, dQG, B, dP, dn_out, dstatus);
  if (rc == MJPL_OK && B == 0) roadmap_reset(e);
  if (rc != MJPL_OK || B == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_roadmap_query(e, *d, dQ, N, dnode_valid, drow_off, dadj, dw, dQI, dQG, B, dP, dn_out, dstatus, dcost);
}

// (the graph is copied to the device with the ends: a caller with many query calls keeps it there and uses the _dev form)
int mjpl_roadmap_query(mjpl_engine *e, const mjpl_roadmap_query_desc *d, const double *Q, int64_t N, const uint8_t *node_valid,
                       const int32_t *row_off, const int32_t *adj, const double *w, const double *QI, const double *QG, int64_t B,
                       double *P, int32_t *n_out, int32_t *status, double *cost) {
  int rc = check_roadmap_query_args(e, d, Q, N, node_valid, row_off, adj, w, QI, QG, B, P, n_out, status);
  if (rc == MJPL_OK && B == 0) roadmap_reset(e);
  if (rc != MJPL_OK || B == 0) return rc;
  const size_t n = (size_t)N, np = e->qidx.size(), qb = (size_t)B * np * sizeof(double), ib = (size_t)B * sizeof(int32_t);
  // (the rows of the graph the search reads: row_off[N] of them; an array that is not a build's reads as an empty graph)
  const size_t m = std::min<size_t>(row_off[n] > 0 ? (size_t)row_off[n] : 0, 2 * n * (size_t)kRmMaxK);
  const HostOut outs[] = {{P, qb * (size_t)d->max_rows}, {n_out, ib}, {status, ib}, {cost, (size_t)B * sizeof(double)}};
  return staged(e, false, {{Q, n * np * sizeof(double)}, {node_valid, n}, {row_off, (n + 1) * sizeof(int32_t)}, {adj, m * sizeof(int32_t)},
                           {w, m * sizeof(double)}, {QI, qb}, {QG, qb}},
                outs, [&](void **in, void **out) {
    return launch_roadmap_query(e, *d, (const double *)in[0], N, (const uint8_t *)in[1], (const int32_t *)in[2], (const int32_t *)in[3],
                                (const double *)in[4], (const double *)in[5], (const double *)in[6], B, (double *)out[0], (int32_t *)out[1],
                                (int32_t *)out[2], (double *)out[3]);
  });
}

// ---- certified edge checks (mjpl_sweep.h)

int mjpl_sweep_bounds(mjpl_engine *e, const double *lo, const double *hi) {
  if (!e) return fail(MJPL_E_ARG, "engine is NULL");
  MJPL_TRY(check_bounds(e, lo, hi));
  HIP_TRY(hipSetDevice(e->device));
  return sweep_use_bounds(e, lo, hi);
}

int mjpl_sweep_measure_dev(mjpl_engine *e, const double *dQ, const double *dHD, int64_t N, int32_t layout, double cap,
                           double *dslack, int32_t *dslack_pair, double *dgap, int32_t *dgap_pair) {
  int rc = check_measure_args(e, dQ, dHD, N, layout, cap, {dslack, dslack_pair, dgap, dgap_pair});
  if (rc != MJPL_OK || N == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_distance(e, DM_SWEEP, dQ, N, layout, cap, nullptr, dgap, dgap_pair, nullptr, nullptr, nullptr, nullptr, 0,
                         nullptr, dHD, dslack, dslack_pair);
}

int mjpl_sweep_measure(mjpl_engine *e, const double *Q, const double *HD, int64_t N, int32_t layout, double cap, double *slack,
                       int32_t *slack_pair, double *gap, int32_t *gap_pair) {
  int rc = check_measure_args(e, Q, HD, N, layout, cap, {slack, slack_pair, gap, gap_pair});
  if (rc != MJPL_OK || N == 0) return rc;
  const size_t n = N, db = sizeof(double), ib = sizeof(int32_t), qb = n * e->qidx.size() * db;
  const HostOut outs[] = {{slack, n * db}, {slack_pair, n * ib}, {gap, n * db}, {gap_pair, n * ib}};
  return staged(e, false, {{Q, qb}, {HD, qb}}, outs, [&](void **in, void **out) {
    return launch_distance(e, DM_SWEEP, (const double *)in[0], N, layout, cap, nullptr, (double *)out[2], (int32_t *)out[3],
                           nullptr, nullptr, nullptr, nullptr, 0, nullptr, (const double *)in[1], (double *)out[0],
                           (int32_t *)out[1]);
  });
}

int mjpl_sweep_edges_dev(mjpl_engine *e, const mjpl_sweep_desc *d, const double *dQA, const double *dQB, int64_t E,
                         int32_t layout, int32_t *dstatus, double *dt_hit, double *dclear_lb, int32_t *dpair, int32_t *dnodes,
                         int32_t *ddepth) {
  int rc = check_sweep_args(e, d, dQA, dQB, E, layout, {dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth});
  if (rc != MJPL_OK || E == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_sweep(e, *d, dQA, dQB, E, layout, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth);
}

int mjpl_sweep_edges(mjpl_engine *e, const mjpl_sweep_desc *d, const double *QA, const double *QB, int64_t E, int32_t layout,
                     int32_t *status, double *t_hit, double *clear_lb, int32_t *pair, int32_t *nodes, int32_t *depth) {
  int rc = check_sweep_args(e, d, QA, QB, E, layout, {status, t_hit, clear_lb, pair, nodes, depth});
  if (rc != MJPL_OK || E == 0) return rc;
  const size_t n = E, db = sizeof(double), ib = sizeof(int32_t), qb = n * e->qidx.size() * db;
  const HostOut outs[] = {{status, n * ib}, {t_hit, n * db}, {clear_lb, n * db}, {pair, n * ib}, {nodes, n * ib}, {depth, n * ib}};
  return staged(e, false, {{QA, qb}, {QB, qb}}, outs, [&](void **in, void **out) {
    return launch_sweep(e, *d, (const double *)in[0], (const double *)in[1], E, layout, (int32_t *)out[0], (double *)out[1],
                        (double *)out[2], (int32_t *)out[3], (int32_t *)out[4], (int32_t *)out[5]);
  });
}

int mjpl_sweep_splines_dev(mjpl_engine *e, const mjpl_sweep_desc *d, const double *dW, const int64_t *wp_off, int64_t B,
                           double *dM, int32_t *dstatus, double *dt_hit, double *dclear_lb, int32_t *dpair, int32_t *dnodes,
                           int32_t *ddepth) {
  int rc = check_spline_sweep_args(e, d, dW, wp_off, B, {dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth});
  if (rc != MJPL_OK || B == 0) return rc;
  HIP_TRY(hipSetDevice(e->device));
  return launch_sweep_splines(e, *d, dW, wp_off, B, dM, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth);
}

int mjpl_sweep_splines(mjpl_engine *e, const mjpl_sweep_desc *d, const double *W, const int64_t *wp_off, int64_t B, double *M,
                       int32_t *status, double *t_hit, double *clear_lb, int32_t *pair, int32_t *nodes, int32_t *depth) {
  int rc = check_spline_sweep_args(e, d, W, wp_off, B, {status, t_hit, clear_lb, pair, nodes, depth});
  if (rc != MJPL_OK || B == 0) return rc;
  const size_t n = (size_t)(wp_off[B] - B), db = sizeof(double), ib = sizeof(int32_t), wb = (size_t)wp_off[B] * e->qidx.size() * db;
  const HostOut outs[] = {{M, wb},         {status, n * ib}, {t_hit, n * db}, {clear_lb, n * db},
                          {pair, n * ib},  {nodes, n * ib},  {depth, n * ib}};
  return staged(e, false, {{W, wb}}, outs, [&](void **in, void **out) {
    return launch_sweep_splines(e, *d, (const double *)in[0], wp_off, B, (double *)out[0], (int32_t *)out[1], (double *)out[2],
                                (double *)out[3], (int32_t *)out[4], (int32_t *)out[5], (int32_t *)out[6]);
  });
}

// ---- memory / stream helpers

int mjpl_dev_alloc(mjpl_engine *e, size_t bytes, void **out) {
  if (!e || !out) return fail(MJPL_E_ARG, "mjpl_dev_alloc: NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
  return MJPL_OK;
}

int mjpl_dev_free(mjpl_engine *e, void *p) {
  if (!e) return fail(MJPL_E_ARG, "mjpl_dev_free: NULL engine");
  HIP_TRY(hipSetDevice(e->device));
  if (p) HIP_TRY(hipFree(p));
  return MJPL_OK;
}

int mjpl_h2d(mjpl_engine *e, void *dst, const void *src, size_t bytes) {
  if (!e || (bytes && (!dst || !src))) return fail(MJPL_E_ARG, "mjpl_h2d: NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
  return MJPL_OK;
}

int mjpl_d2h(mjpl_engine *e, void *dst, const void *src, size_t bytes) {
  if (!e || (bytes && (!dst || !src))) return fail(MJPL_E_ARG, "mjpl_d2h: NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
  return MJPL_OK;
}

int mjpl_sync(mjpl_engine *e) {
  if (!e) return fail(MJPL_E_ARG, "mjpl_sync: NULL engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  return MJPL_OK;
}

void *mjpl_stream(mjpl_engine *e) { return e ? (void *)e->stream : nullptr; }

// ---- measurement: per-launch HIP-event timing on the engine's own stream

int mjpl_time_edges_stages_dev(mjpl_engine *e, const double *dQA, const double *dQB, int64_t E, double step_dist,
                               int32_t layout, uint8_t *dvalid, int32_t iters, int32_t sample_every,
                               float *ms_mean, float *stage_ms, int32_t *nsamples) {
  if (!e || iters < 0 || (iters > 0 && !ms_mean)) return fail(MJPL_E_ARG, "mjpl_time_edges_stages_dev: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  if (sample_every < 1) sample_every = 1;
  // Two events around the whole run (the mean step) and, on every `sample_every`-th step, one
  // event after each stage of the launch: bracketing every kernel of every step would cost a few
  // percent of the throughput the run is there to measure.
  // (sample_every > iters: NO launch is bracketed -- a bracketed launch costs ~56 us more than a plain one, 1.4 % of a
  //  20-step region: bench.py takes the per-kernel durations of such a region from launches outside it)
  const bool none = sample_every > iters;
  const int nsamp = (iters > 0 && !none) ? (iters + sample_every - 1) / sample_every : 0;
  constexpr int NM = MJPL_NSTAGES + 1;
  std::vector<hipEvent_t> ev((size_t)nsamp * NM + 2);
  for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
  hipEvent_t region_start = ev[(size_t)nsamp * NM], region_end = ev[(size_t)nsamp * NM + 1];
  int rc = MJPL_OK;
  HIP_TRY(hipEventRecord(region_start, e->stream));
  for (int k = 0; k < iters && rc == MJPL_OK; k++) {
    e->marks = (!none && k % sample_every == 0) ? &ev[(size_t)(k / sample_every) * NM] : nullptr;
    rc = mjpl_check_edges_dev(e, dQA, dQB, E, step_dist, layout, 0, dvalid, nullptr);
    e->marks = nullptr;
  }
  HIP_TRY(hipEventRecord(region_end, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  if (rc == MJPL_OK && iters > 0) {
    float total = 0;
    HIP_TRY(hipEventElapsedTime(&total, region_start, region_end));
    *ms_mean = total / (float)iters;
    if (stage_ms && nsamp > 0) {
      for (int st = 0; st < MJPL_NSTAGES; st++) {
        double acc = 0;
        for (int sidx = 0; sidx < nsamp; sidx++) {
          float t = 0;
          HIP_TRY(hipEventElapsedTime(&t, ev[(size_t)sidx * NM + st], ev[(size_t)sidx * NM + st + 1]));
          acc += t;
        }
        stage_ms[st] = (float)(acc / nsamp);
      }
    }
    if (nsamples) *nsamples = nsamp;
  }
  for (auto &x : ev) (void)hipEventDestroy(x);
  return rc;
}

int mjpl_time_edges_dev(mjpl_engine *e, const double *dQA, const double *dQB, int64_t E, double step_dist,
                        int32_t layout, uint8_t *dvalid, int32_t iters, float *ms, float *ms_first) {
  if (!e || iters < 0 || (iters > 0 && !ms)) return fail(MJPL_E_ARG, "mjpl_time_edges_dev: bad argument");
  float mean = 0, stage[MJPL_NSTAGES] = {0};
  const int rc = mjpl_time_edges_stages_dev(e, dQA, dQB, E, step_dist, layout, dvalid, iters, 1, &mean,
                                            ms_first ? stage : nullptr, nullptr);
  if (rc != MJPL_OK) return rc;
  const int main_stage = (e->filter && e->fb.usable) ? MJPL_STAGE_ITEMS : MJPL_STAGE_EXACT;
  for (int k = 0; k < iters; k++) {
    ms[k] = mean;
    if (ms_first) ms_first[k] = stage[main_stage];
  }
  return MJPL_OK;
}

int mjpl_time_configs_dev(mjpl_engine *e, const double *dQ, int64_t N, int32_t layout, uint8_t *dvalid,
                          int32_t iters, float *ms) {
  if (!e || iters < 0 || (iters > 0 && !ms)) return fail(MJPL_E_ARG, "mjpl_time_configs_dev: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  std::vector<hipEvent_t> ev(2 * (size_t)iters);
  for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
  int rc = MJPL_OK;
  for (int k = 0; k < iters && rc == MJPL_OK; k++) {
    HIP_TRY(hipEventRecord(ev[2 * k], e->stream));
    rc = mjpl_check_configs_dev(e, dQ, N, layout, dvalid);
    HIP_TRY(hipEventRecord(ev[2 * k + 1], e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < iters && rc == MJPL_OK; k++) HIP_TRY(hipEventElapsedTime(&ms[k], ev[2 * k], ev[2 * k + 1]));
  for (auto &x : ev) (void)hipEventDestroy(x);
  return rc;
}

int mjpl_time_topp_dev(mjpl_engine *e, const mjpl_topp_desc *d, const double *dW, const int64_t *wp_off, int64_t B, double *dM,
                       double *dx, double *du, double *dt_grid, int32_t *dstatus, double dt, const int64_t *samp_off, double *dpos,
                       double *dvel, double *dacc, int32_t iters, float *ms_profile, float *ms_sample) {
  if (!e || iters < 0 || (iters > 0 && (!ms_profile || !ms_sample))) return fail(MJPL_E_ARG, "mjpl_time_topp_dev: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  std::vector<hipEvent_t> ev(3 * (size_t)iters);
  for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
  int rc = MJPL_OK;
  for (int k = 0; k < iters && rc == MJPL_OK; k++) {
    HIP_TRY(hipEventRecord(ev[3 * k], e->stream));
    rc = mjpl_topp_profile_dev(e, d, dW, wp_off, B, dM, dx, du, dt_grid, dstatus);
    HIP_TRY(hipEventRecord(ev[3 * k + 1], e->stream));
    if (rc == MJPL_OK) rc = mjpl_topp_sample_dev(e, d, dW, wp_off, B, dM, dx, du, dt_grid, dt, samp_off, dpos, dvel, dacc);
    HIP_TRY(hipEventRecord(ev[3 * k + 2], e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < iters && rc == MJPL_OK; k++) {
    HIP_TRY(hipEventElapsedTime(&ms_profile[k], ev[3 * k], ev[3 * k + 1]));
    HIP_TRY(hipEventElapsedTime(&ms_sample[k], ev[3 * k + 1], ev[3 * k + 2]));
  }
  for (auto &x : ev) (void)hipEventDestroy(x);
  return rc;
}

int mjpl_time_jerk_dev(mjpl_engine *e, const mjpl_jerk_desc *d, const double *dW, const int64_t *wp_off, int64_t B, double *dM,
                       double *dlim, double *dv, double *dvp, double *dtc, double *dt_grid, int32_t *dstatus, double dt,
                       const int64_t *samp_off, double *dpos, double *dvel, double *dacc, int32_t iters, float *ms_profile,
                       float *ms_sample) {
  if (!e || iters < 0 || (iters > 0 && (!ms_profile || !ms_sample))) return fail(MJPL_E_ARG, "mjpl_time_jerk_dev: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  std::vector<hipEvent_t> ev(3 * (size_t)iters);
  for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
  int rc = MJPL_OK;
  for (int k = 0; k < iters && rc == MJPL_OK; k++) {
    HIP_TRY(hipEventRecord(ev[3 * k], e->stream));
    rc = mjpl_jerk_profile_dev(e, d, dW, wp_off, B, dM, dlim, dv, dvp, dtc, dt_grid, dstatus);
    HIP_TRY(hipEventRecord(ev[3 * k + 1], e->stream));
    if (rc == MJPL_OK) rc = mjpl_jerk_sample_dev(e, d, dW, wp_off, B, dM, dlim, dv, dvp, dtc, dt_grid, dt, samp_off, dpos, dvel, dacc);
    HIP_TRY(hipEventRecord(ev[3 * k + 2], e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < iters && rc == MJPL_OK; k++) {
    HIP_TRY(hipEventElapsedTime(&ms_profile[k], ev[3 * k], ev[3 * k + 1]));
    HIP_TRY(hipEventElapsedTime(&ms_sample[k], ev[3 * k + 1], ev[3 * k + 2]));
  }
  for (auto &x : ev) (void)hipEventDestroy(x);
  return rc;
}

int mjpl_time_sweep_dev(mjpl_engine *e, const mjpl_sweep_desc *d, const double *dA, double *dB, const int64_t *wp_off, int64_t n,
                        int32_t layout, int32_t *dstatus, double *dt_hit, double *dclear_lb, int32_t *dpair, int32_t *dnodes,
                        int32_t *ddepth, int32_t iters, float *ms) {
  if (!e || iters < 0 || (iters > 0 && !ms)) return fail(MJPL_E_ARG, "mjpl_time_sweep_dev: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  std::vector<hipEvent_t> ev(2 * (size_t)iters);
  for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
  int rc = MJPL_OK;
  for (int k = 0; k < iters && rc == MJPL_OK; k++) {
    HIP_TRY(hipEventRecord(ev[2 * k], e->stream));
    rc = wp_off ? mjpl_sweep_splines_dev(e, d, dA, wp_off, n, dB, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth)
                : mjpl_sweep_edges_dev(e, d, dA, dB, n, layout, dstatus, dt_hit, dclear_lb, dpair, dnodes, ddepth);
    HIP_TRY(hipEventRecord(ev[2 * k + 1], e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < iters && rc == MJPL_OK; k++) HIP_TRY(hipEventElapsedTime(&ms[k], ev[2 * k], ev[2 * k + 1]));
  for (auto &x : ev) (void)hipEventDestroy(x);
  return rc;
}

// ---- row f1: PoseConstraint ---------------------------------------------------------------

struct mjpl_pose {
  mjpl_engine *e = nullptr;
  std::vector<int> pi;
  std::vector<double> pd;
  int *d_pi = nullptr;
  double *d_pd = nullptr;
  int nq = 0, nj = 0;
  uint64_t chain_hash = 0;  // of the chain program (bodies, joints, their constants): names a generated projection
  bool spec_off = false;    // MJPL_POSE_SPEC=0 at creation: the interpreting kernels whatever the engine has loaded
};

namespace {
size_t pose_lds(const mjpl_pose *p) { return (size_t)kPoseBlock * sizeof(double) * ((size_t)p->nq + 6 * (size_t)p->nj); }

int pose_check(const mjpl_pose *p, const void *a, int64_t n) {
  if (!p) return fail(MJPL_E_ARG, "pose handle is NULL");
  if (n < 0) return fail(MJPL_E_ARG, "negative batch size");
  if (n > 0 && !a) return fail(MJPL_E_ARG, "NULL batch pointer");
  return MJPL_OK;
}

// How a batch of N rows (projections, IK seeds, active planner lanes) goes to the row kernels of mjpl_rows.h.  The
// kernels hold one wave per SIMD (their registers), 1 024 waves on the chip.  While ALL rows can be resident at once
// a row gets as many lanes as that allows -- eight up to 8 192 rows, four up to 16 384 (the lanes split a third of a
// Newton step's instructions) -- and every row starts with the launch: such batches are bound by their slowest row,
// which must not wait for a free lane first.  Beyond that one lane per row, and a wave owns ceil(N / 1 024) >= 64 rows:
// it refills as rows end.  Option "rows_g": force the lanes per row (A/B timing).
struct RowsShape { int G; unsigned grid; int64_t per; };
RowsShape rows_shape(int64_t N, int forced = 0) {  // (forced: option "rows_g" -- tests compare the three kernels on one batch)
  const int64_t max_waves = 1024;  // one per SIMD: what the row kernels' registers allow (mjpl_rows.h)
  RowsShape r;
  r.G = N <= 8 * max_waves ? 8 : (N <= 16 * max_waves ? 4 : 1);
  if (forced == 1 || forced == 4 || forced == 8) r.G = forced;
  const int64_t rows_per_wave = 64 / r.G;
  const int64_t waves = std::min<int64_t>(max_waves, (N + rows_per_wave - 1) / rows_per_wave);
  r.per = (N + waves - 1) / waves;
  r.grid = (unsigned)((N + r.per - 1) / r.per);
  return r;
}

// the generated projection of this handle's chain in the library its engine has loaded NOW (set_planning may have
// changed it since the handle was made), or -1
int pose_spec_index(const mjpl_pose *p) {
  const SpecLib *sl = p->e->spec;
  if (!sl || p->spec_off) return -1;
  for (int k = 0; k < sl->pose_count; k++)
    if (sl->pose_hash(k) == p->chain_hash) return k;
  return -1;
}
}  // namespace

// Host only, no device needed: the chain program of (model, site body) -- what mjpl_pose_create compiles and
// mjpl_amd/specialise.py turns into straight-line code -- and its hash.  Call with pi = pd = NULL for the sizes.
int mjpl_pose_chain_dump(const mjpl_model_desc *d, int32_t site_body, int32_t *pi, int32_t *npi, double *pd, int32_t *npd,
                         uint64_t *hash) {
  if (!d || !npi || !npd || !hash) return fail(MJPL_E_ARG, "mjpl_pose_chain_dump: NULL argument");
  if (d->nq != d->njnt) return fail(MJPL_E_JOINT, "nq != njnt: only 1-DoF joints are supported");
  std::unique_ptr<mjpl_engine> e(new mjpl_engine());
  int rc = engine_from_desc(e.get(), d, nullptr, 0);
  if (rc != MJPL_OK) return rc;
  if (site_body < 0 || site_body >= e->m.nbody) return fail(MJPL_E_ARG, "site body %d out of range", site_body);
  std::vector<int> vi;
  std::vector<double> vd;
  int nj = 0;
  if ((rc = build_chain(e->m, site_body, vi, vd, &nj)) != MJPL_OK) return rc;
  *hash = chain_hash_of(vi, vd, vd.size());
  const bool fits = pi && pd && *npi >= (int32_t)vi.size() && *npd >= (int32_t)vd.size();
  *npi = (int32_t)vi.size();
  *npd = (int32_t)vd.size();
  if (fits) {
    memcpy(pi, vi.data(), vi.size() * sizeof(int));
    memcpy(pd, vd.data(), vd.size() * sizeof(double));
  }
  return MJPL_OK;
}

// 0: the interpreting kernels serve this handle; 1: a generated projection of the engine's library does
int mjpl_pose_spec_loaded(mjpl_pose *p) { return (p && pose_spec_index(p) >= 0) ? 1 : 0; }

int mjpl_pose_create(mjpl_engine *e, const mjpl_pose_desc *d, mjpl_pose **out) {
  if (!e || !d || !out) return fail(MJPL_E_ARG, "mjpl_pose_create: NULL argument");
  const HostModel &m = e->m;
  if (d->site_body < 0 || d->site_body >= m.nbody) return fail(MJPL_E_ARG, "site body %d out of range", d->site_body);
  if (!d->jnt_range) return fail(MJPL_E_ARG, "jnt_range is NULL");
  if (d->tolerance < 0.0) return fail(MJPL_E_ARG, "`tolerance` must be >= 0.");
  if (!(d->q_step > 0.0)) return fail(MJPL_E_ARG, "`q_step` must be > 0.");
  if (m.nq != m.njnt) return fail(MJPL_E_JOINT, "pose projection needs 1-DoF joints only (nq %d != njnt %d)", m.nq, m.njnt);
  auto p = std::make_unique<mjpl_pose>();
  p->e = e;
  p->nq = m.nq;
  int rc = build_chain(m, d->site_body, p->pi, p->pd, &p->nj);
  if (rc != MJPL_OK) return rc;
  p->chain_hash = chain_hash_of(p->pi, p->pd, p->pd.size());
  p->spec_off = e->pose_spec == 0;  // (option "pose_spec")
  p->pi[PH_MAXIT] = d->max_iters > 0 ? d->max_iters : 1000;
  p->pi[PH_OFF_TAIL] = (int)p->pd.size();
  p->pd.resize(p->pd.size() + PT_SIZE);
  double *t = p->pd.data() + p->pi[PH_OFF_TAIL];
  for (int k = 0; k < 3; k++) { t[PT_SITE_POS + k] = d->site_pos[k]; t[PT_C_POS + k] = d->c_pos[k]; }
  for (int k = 0; k < 4; k++) { t[PT_SITE_QUAT + k] = d->site_quat[k]; t[PT_C_QUAT + k] = d->c_quat[k]; }
  for (int k = 0; k < 6; k++) { t[PT_LO + k] = d->lo[k]; t[PT_HI + k] = d->hi[k]; }
  t[PT_TOL] = d->tolerance;
  t[PT_QSTEP] = d->q_step;
  p->pi[PH_OFF_JRANGE] = (int)p->pd.size();
  for (int k = 0; k < 2 * m.njnt; k++) p->pd.push_back(d->jnt_range[k]);
  if (pose_lds(p.get()) > 64 * 1024)
    return fail(MJPL_E_CAPACITY, "pose projection: %d qpos + %d chain joints exceed the LDS budget", p->nq, p->nj);
  HIP_TRY(hipSetDevice(e->device));
  MJPL_TRY(upload_table(&p->d_pi, p->pi));
  MJPL_TRY(upload_table(&p->d_pd, p->pd));
  *out = p.release();
  return MJPL_OK;
}

void mjpl_pose_destroy(mjpl_pose *p) {
  if (!p) return;
  (void)hipSetDevice(p->e->device);
  if (p->d_pi) (void)hipFree(p->d_pi);
  if (p->d_pd) (void)hipFree(p->d_pd);
  delete p;
}

int mjpl_pose_set_q_step(mjpl_pose *p, double q_step) {
  if (!p) return fail(MJPL_E_ARG, "pose handle is NULL");
  if (!(q_step > 0.0)) return fail(MJPL_E_ARG, "`q_step` must be > 0.");
  const size_t at = (size_t)p->pi[PH_OFF_TAIL] + PT_QSTEP;
  p->pd[at] = q_step;
  HIP_TRY(hipSetDevice(p->e->device));
  HIP_TRY(hipStreamSynchronize(p->e->stream));
  HIP_TRY(hipMemcpy(p->d_pd + at, &p->pd[at], sizeof(double), hipMemcpyHostToDevice));
  return MJPL_OK;
}

int mjpl_pose_apply_dev(mjpl_pose *p, const double *dQold, const double *dQ, int64_t N, double *dQout,
                        uint8_t *dok, int32_t *diters) {
  int rc = pose_check(p, dQ, N);
  if (rc != MJPL_OK) return rc;
  if (N == 0) return MJPL_OK;
  if (!dQold || !dQout || !dok) return fail(MJPL_E_ARG, "NULL pointer");
  HIP_TRY(hipSetDevice(p->e->device));
  KtScope kt_scope(p->e, 1);  // (option "kernel_timer")
  const unsigned grid = (unsigned)((N + kPoseBlock - 1) / kPoseBlock);
  const int k = pose_spec_index(p);
  if (k >= 0) {
    mjpl_engine *e = p->e;
    const RowsShape rs = rows_shape(N, e->rows_g);
    // MJPL_POSE_PHASE_STEPS=k (an experiment, off by default): a batch too large for several lanes per row in two
    // launches (mjpl_rows.h: PosePhase) -- every row's first k Newton steps with one lane per row, then the rows that
    // want more, a list the first launch packs, with eight.  Same bytes; measured SLOWER at 131 072 rows (0.198 ms in
    // one launch; k = 2 / 3 / 4 / 6: 0.352 / 0.283 / 0.247 / 0.206 -- profiles/r05h_pose_phase.json): eight lanes per row
    // cost eight times the lanes for 1.6 times the speed, and 40 % of the rows want more than three steps.
    const int phase_steps = e->pose_phase_steps;  // (option "pose_phase_steps")
    if (rs.G == 1 && phase_steps > 0) {
      const size_t need = ((size_t)N * 2 + 16) * sizeof(int32_t);
      if ((rc = e->stage_parked.reserve(need, kStageFloor)) != MJPL_OK) return rc;
      int32_t *list = (int32_t *)e->stage_parked.p, *itst = list + N;
      int *count = (int *)(itst + N);
      HIP_TRY(hipMemsetAsync(count, 0, sizeof(int), e->stream));
      const PosePhase first = {phase_steps, nullptr, nullptr, list, count, itst};
      int rc2 = e->spec->pose_apply(k, 1, e->stream, rs.grid, p->d_pi, p->d_pd, dQold, dQ, N, rs.per, dQout, dok, diters, first);
      if (rc2 == 0) {
        const PosePhase second = {0, list, count, nullptr, nullptr, itst};
        rc2 = e->spec->pose_apply(k, 8, e->stream, 1024u, p->d_pi, p->d_pd, dQold, dQ, N, 0, dQout, dok, diters, second);
        if (rc2 == 0) return MJPL_OK;
        return fail(MJPL_E_HIP, "generated projection kernel (second launch) failed to launch");
      }
      if (rc2 != -1) return fail(MJPL_E_HIP, "generated projection kernel failed to launch");
    } else {
      const PosePhase whole = {0, nullptr, nullptr, nullptr, nullptr, nullptr};
      const int rc2 = e->spec->pose_apply(k, rs.G, e->stream, rs.grid, p->d_pi, p->d_pd, dQold, dQ, N, rs.per, dQout, dok, diters, whole);
      if (rc2 == 0) return MJPL_OK;
      if (rc2 != -1) return fail(MJPL_E_HIP, "generated projection kernel failed to launch");
    }
  }
  hipLaunchKernelGGL(k_pose_apply, dim3(grid), dim3(kPoseBlock), pose_lds(p), p->e->stream, p->d_pi, p->d_pd,
                     dQold, dQ, N, dQout, dok, diters);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

int mjpl_pose_valid_dev(mjpl_pose *p, const double *dQ, int64_t N, uint8_t *dvalid, double *dxpos, double *dxmat) {
  int rc = pose_check(p, dQ, N);
  if (rc != MJPL_OK) return rc;
  if (N == 0) return MJPL_OK;
  HIP_TRY(hipSetDevice(p->e->device));
  const unsigned grid = (unsigned)((N + kPoseBlock - 1) / kPoseBlock);
  hipLaunchKernelGGL(k_pose_valid, dim3(grid), dim3(kPoseBlock), (size_t)kPoseBlock * sizeof(double) * p->nq,
                     p->e->stream, p->d_pi, p->d_pd, dQ, N, dvalid, dxpos, dxmat);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

int mjpl_pose_apply(mjpl_pose *p, const double *Q_old, const double *Q, int64_t N, double *Q_out,
                    uint8_t *ok, int32_t *iters) {
  int rc = pose_check(p, Q, N);
  if (rc != MJPL_OK) return rc;
  if (N == 0) return MJPL_OK;
  if (!Q_old || !Q_out || !ok) return fail(MJPL_E_ARG, "NULL pointer");
  const size_t n = N, qb = n * p->nq * sizeof(double);
  return staged(p->e, false, {{Q_old, qb}, {Q, qb}}, {{Q_out, qb}, {ok, n}, {iters, n * sizeof(int32_t)}},
                [&](void **in, void **out) {
                  return mjpl_pose_apply_dev(p, (const double *)in[0], (const double *)in[1], N, (double *)out[0],
                                             (uint8_t *)out[1], (int32_t *)out[2]);
                });
}

int mjpl_pose_valid(mjpl_pose *p, const double *Q, int64_t N, uint8_t *valid, double *xpos, double *xmat) {
  int rc = pose_check(p, Q, N);
  if (rc != MJPL_OK) return rc;
  if (N == 0) return MJPL_OK;
  const size_t n = N, db = sizeof(double);
  return staged(p->e, false, {{Q, n * p->nq * db}}, {{valid, n}, {xpos, n * 3 * db}, {xmat, n * 9 * db}},
                [&](void **in, void **out) {
                  return mjpl_pose_valid_dev(p, (const double *)in[0], N, (uint8_t *)out[0], (double *)out[1],
                                             (double *)out[2]);
                });
}

// ---- planning in lockstep under a PoseConstraint (mjpl_cplan.h)

namespace {
int check_cplan_args(const mjpl_pose *p, const mjpl_cplan_desc *d, int extend, const void *QI, const void *QG, int64_t B,
                     const double *lo, const double *hi, const void *P, const void *n_out, const void *status) {
  if (extend < 1 || extend > kCplanMaxExtend) return fail(MJPL_E_ARG, "`extend` must be 1..%d, got %d", kCplanMaxExtend, extend);
  if (!p) return fail(MJPL_E_ARG, "pose handle is NULL");
  if (!d) return fail(MJPL_E_ARG, "mjpl_plan: NULL descriptor");
  const mjpl_plan_desc pd = {d->epsilon, d->step_dist, d->seed, d->rounds, d->candidates, d->nodes, 0};
  if (d->chain < 1 || d->chain > kCplanMaxChain) return fail(MJPL_E_ARG, "`chain` must be 1..%d, got %d", kCplanMaxChain, d->chain);
  if (d->max_rows < 2) return fail(MJPL_E_ARG, "`max_rows` must be >= 2, got %d", d->max_rows);
  const size_t np = p->e->qidx.size();
  if (np < 1 || np > (size_t)kRrtMaxPlan) return fail(MJPL_E_ARG, "%zu planning columns (1..%d supported under a projection)", np, kRrtMaxPlan);
  return check_plan_args(p->e, &pd, QI, QG, B, lo, hi, P, n_out, status);
}

size_t cplan_lds(const mjpl_pose *p) { return pose_lds(p) + (size_t)kPoseBlock * sizeof(double) * ((size_t)p->nq + p->e->qidx.size()); }

// carve_plan, and what the projection adds: the extension chains' links (X to a lane) and their counts, the bridge's
// links (S), the ends as full rows.  The ends' verdicts are 4 nb bytes: the launcher splits them.
void carve_cplan(Carver &c, size_t nb, size_t emax, size_t X, size_t S, size_t N, size_t np, size_t nq, size_t scan_bytes, CplanBatch *a,
                 RoundSpans *s) {
  const size_t L64 = kPlanLanes;
  carve_plan(c, nb, emax, 4 * nb, N, np, scan_bytes, a, s);
  a->cy = c.take<double>(nb * X * np * L64);
  a->cl = c.take<double>(nb * S * np);
  a->cfq = c.take<double>(2 * nb * nq);
  a->cn = c.take<int>(nb * L64);
  a->nlinks = c.take<int>(nb);
}

// mjpl_plan_paths_constrained* on device batches (lo, hi on the host), an extension a chain of up to `extend` steps.
// Per chunk of problems whose workspace fits the option "plan_chunk_bytes" (always at least one problem): k_cplan_init,
// ONE launch_configs and ONE k_pose_valid on the ends, the chunk's rounds (run_rounds) -- a round proposes, projects
// and counts -- then k_cplan_finish.
int launch_cplan(mjpl_pose *p, const mjpl_cplan_desc &d, int extend, const double *dQI, const double *dQG, int64_t B,
                 const double *lo, const double *hi, double *dP, int32_t *dn_out, int32_t *dstatus, int32_t *drounds_used, int32_t *dedges,
                 int32_t *dtree_nodes) {
  mjpl_engine *e = p->e;
  plan_reset(e);
  if (cplan_lds(p) > 64 * 1024)
    return fail(MJPL_E_CAPACITY, "constrained planning: %d qpos + %d chain joints exceed the LDS budget", p->nq, p->nj);
  const hipStream_t st = e->stream;
  HIP_TRY(hipStreamSynchronize(st));  // (an earlier call's launches read the same buffers)
  const size_t np = e->qidx.size(), nq = (size_t)p->nq, K = (size_t)d.candidates, N = (size_t)d.nodes, S = (size_t)d.chain,
               X = (size_t)extend, L64 = kPlanLanes;
  const size_t per_edges = S + 1 + K * X;  // a problem's edges in one round at most: the bridge, then K chains of X links
  // the sampling box and the base configuration; the planning columns and their inverse
  std::vector<int> qmap(np + nq, -1);
  for (size_t c = 0; c < np; c++) {
    qmap[c] = e->qidx[c];
    qmap[np + (size_t)e->qidx[c]] = (int)c;
  }
  MJPL_TRY(e->d_pl_box.reserve(2 * np + nq, 64));
  MJPL_TRY(e->d_pl_q.reserve(np + nq, 64));
  MJPL_TRY(e->d_pl_head.reserve(4));
  HIP_TRY(hipMemcpyAsync(e->d_pl_box.p, lo, np * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->d_pl_box.p + np, hi, np * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->d_pl_box.p + 2 * np, e->qbase.data(), nq * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(e->d_pl_q.p, qmap.data(), (np + nq) * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));  // (qmap is pageable and leaves scope with this call)
  HIP_TRY(hipMemsetAsync(dP, 0, (size_t)B * (size_t)d.max_rows * np * sizeof(double), st));
  // what one problem adds to a chunk: two trees with their parents, S + 1 + K X edges (two rows and a verdict each), the
  // round's targets, the extension chains' links (X to a lane) and the bridge's, the nodes they step from, its two ends
  // (planning and full rows), its counters
  const size_t per_problem = 2 * N * (np * sizeof(double) + sizeof(int)) + per_edges * (2 * np * sizeof(double) + 1) +
                             L64 * ((1 + X) * np * sizeof(double) + 2 * sizeof(int)) + S * np * sizeof(double) +
                             2 * (np + nq) * sizeof(double) + 20 * sizeof(int);
  const size_t fit = std::max<size_t>((size_t)e->plan_chunk_bytes / per_problem, 1);
  const size_t chunk = std::min(fit, ((size_t)1 << 30) / per_edges);  // (edge offsets are ints)
  PhaseLog phases;
  CplanBatch a = {};
  a.QI = dQI; a.QG = dQG; a.box = e->d_pl_box.p; a.qbase = e->d_pl_box.p + 2 * np;
  a.qidx = e->d_pl_q.p; a.qinv = e->d_pl_q.p + np; a.pi = p->d_pi; a.pd = p->d_pd; a.nq = p->nq;
  a.d = (int)np; a.K = d.candidates; a.N = d.nodes; a.R = d.rounds; a.S = d.chain; a.X = extend; a.max_rows = d.max_rows;
  a.epsilon = d.epsilon;
  a.seed_mixed = shortcut_mix(d.seed);
  a.head = e->d_pl_head.p;
  a.P = dP; a.n_out = dn_out; a.status = dstatus; a.rounds_used = drounds_used; a.edges = dedges; a.tree_nodes = dtree_nodes;
  for (int64_t b0 = 0; b0 < B; b0 += (int64_t)chunk) {
    const size_t nb = std::min(chunk, (size_t)(B - b0));
    size_t scan_bytes = 0;
    MJPL_TRY(scan_space(st, nb + 1, &scan_bytes));
    RoundSpans s = {};
    MJPL_TRY(carve_arena(e->d_pl_arena, [&](Carver &c) { carve_cplan(c, nb, nb * per_edges, X, S, N, np, nq, scan_bytes, &a, &s); }));
    a.b0 = (int)b0; a.nb = (int)nb;
    uint8_t *const pose_valid = s.valid + 2 * nb;  // the ends' verdicts: the configurations' first, then the poses'
    a.pvalid = pose_valid;
    const dim3 grid((unsigned)((nb + kPlanWaves - 1) / kPlanWaves)), block(64 * kPlanWaves);
    const int chain_blocks = (int)((nb + kPoseBlock - 1) / kPoseBlock);
    const dim3 pgrid((unsigned)(chain_blocks + (nb * K + kPoseBlock - 1) / kPoseBlock));
    MJPL_TRY(launch_checked(st, k_cplan_init, grid, block, 0, a));
    MJPL_TRY(launch_configs(e, a.cfg, (int64_t)(2 * nb), MJPL_AOS, s.valid, nullptr));
    MJPL_TRY(mjpl_pose_valid_dev(p, a.cfq, (int64_t)(2 * nb), pose_valid, nullptr, nullptr));
    MJPL_TRY(run_rounds(
        e, phases, s, 0, d.rounds, d.step_dist, &e->plan_last_rounds, &e->plan_last_edges,
        [&](int r) {
          a.round = r;
          return launch_checked(st, k_cplan_propose, grid, block, 0, a);
        },
        [&](int) {
          {
            PhaseScope ph(e, phases, 3);
            MJPL_TRY(launch_checked(st, k_cplan_project, pgrid, dim3(kPoseBlock), cplan_lds(p), a, chain_blocks));
          }
          PhaseScope ph(e, phases, 0);
          return launch_checked(st, k_cplan_count, grid, block, 0, a);
        },
        [&] { return launch_checked(st, k_cplan_gather, grid, block, 0, a); },
        [&](int) { return launch_checked(st, k_cplan_commit, grid, block, 0, a); }));
    MJPL_TRY(launch_checked(st, k_cplan_finish, grid, block, 0, a));
    e->plan_last_chunks++;
  }
  // an edge the edge kernels refuse counts as invalid here: the pipeline's status word is not this call's to report
  HIP_TRY(hipMemsetAsync(e->d_status, 0, sizeof(int), st));
  return phase_sums(e, phases, e->plan_last_ms);
}
}  // namespace

int mjpl_plan_paths_constrained_ext_dev(mjpl_pose *p, const mjpl_cplan_desc *d, int32_t extend, const double *dQI, const double *dQG,
                                        int64_t B, const double *lo, const double *hi, double *dP, int32_t *dn_out, int32_t *dstatus,
                                        int32_t *drounds_used, int32_t *dedges, int32_t *dtree_nodes) {
  int rc = check_cplan_args(p, d, extend, dQI, dQG, B, lo, hi, dP, dn_out, dstatus);
  if (rc == MJPL_OK && B == 0) plan_reset(p->e);
  if (rc != MJPL_OK || B == 0) return rc;
  HIP_TRY(hipSetDevice(p->e->device));
  return launch_cplan(p, *d, extend, dQI, dQG, B, lo, hi, dP, dn_out, dstatus, drounds_used, dedges, dtree_nodes);
}

int mjpl_plan_paths_constrained_ext(mjpl_pose *p, const mjpl_cplan_desc *d, int32_t extend, const double *QI, const double *QG,
                                    int64_t B, const double *lo, const double *hi, double *P, int32_t *n_out, int32_t *status,
                                    int32_t *rounds_used, int32_t *edges, int32_t *tree_nodes) {
  int rc = check_cplan_args(p, d, extend, QI, QG, B, lo, hi, P, n_out, status);
  if (rc == MJPL_OK && B == 0) plan_reset(p->e);
  if (rc != MJPL_OK || B == 0) return rc;
  mjpl_engine *e = p->e;
  const size_t qb = (size_t)B * e->qidx.size() * sizeof(double), ib = (size_t)B * sizeof(int32_t);
  const HostOut outs[] = {{P, qb * (size_t)d->max_rows}, {n_out, ib}, {status, ib}, {rounds_used, ib}, {edges, ib}, {tree_nodes, 2 * ib}};
  return staged(e, false, {{QI, qb}, {QG, qb}}, outs, [&](void **in, void **out) {
    return launch_cplan(p, *d, extend, (const double *)in[0], (const double *)in[1], B, lo, hi, (double *)out[0],
                        (int32_t *)out[1], (int32_t *)out[2], (int32_t *)out[3], (int32_t *)out[4], (int32_t *)out[5]);
  });
}

int mjpl_plan_paths_constrained_dev(mjpl_pose *p, const mjpl_cplan_desc *d, const double *dQI, const double *dQG, int64_t B,
                                    const double *lo, const double *hi, double *dP, int32_t *dn_out, int32_t *dstatus,
                                    int32_t *drounds_used, int32_t *dedges, int32_t *dtree_nodes) {
  return mjpl_plan_paths_constrained_ext_dev(p, d, 1, dQI, dQG, B, lo, hi, dP, dn_out, dstatus, drounds_used, dedges, dtree_nodes);
}

int mjpl_plan_paths_constrained(mjpl_pose *p, const mjpl_cplan_desc *d, const double *QI, const double *QG, int64_t B,
                                const double *lo, const double *hi, double *P, int32_t *n_out, int32_t *status, int32_t *rounds_used,
                                int32_t *edges, int32_t *tree_nodes) {
  return mjpl_plan_paths_constrained_ext(p, d, 1, QI, QG, B, lo, hi, P, n_out, status, rounds_used, edges, tree_nodes);
}

// ---- row f3: IK seeds ------------------------------------------------------------------------


int mjpl_ik_solve_dev(mjpl_engine *e, const mjpl_ik_desc *d, const double *dQ, int64_t N, double *dQout,
                      uint8_t *dok, int32_t *diters, double *derr) {
  if (!e || !d) return fail(MJPL_E_ARG, "mjpl_ik_solve: NULL argument");
  if (N < 0) return fail(MJPL_E_ARG, "negative batch size");
  if (N == 0) return MJPL_OK;
  if (!dQ || !dQout || !dok) return fail(MJPL_E_ARG, "NULL pointer");
  const HostModel &m = e->m;
  if (d->site_body < 0 || d->site_body >= m.nbody) return fail(MJPL_E_ARG, "site body %d out of range", d->site_body);
  if (!d->jnt_range || !d->movable) return fail(MJPL_E_ARG, "jnt_range / movable is NULL");
  if (d->iterations < 1) return fail(MJPL_E_ARG, "`iterations` must be > 0.");
  if (m.nq != m.njnt) return fail(MJPL_E_JOINT, "IK needs 1-DoF joints only (nq %d != njnt %d)", m.nq, m.njnt);
  std::vector<int> pi;
  std::vector<double> pd;
  int nj = 0;
  int rc = build_chain(m, d->site_body, pi, pd, &nj);
  if (rc != MJPL_OK) return rc;
  // the chain as straight-line code, if the engine's library has it (same results; MJPL_POSE_SPEC=0: interpreted)
  int spec_k = -1;
  {
    if (e->spec && e->spec->pose_count > 0 && e->pose_spec != 0) {
      const uint64_t h = chain_hash_of(pi, pd, pd.size());
      for (int k = 0; k < e->spec->pose_count && spec_k < 0; k++)
        if (e->spec->pose_hash(k) == h) spec_k = k;
    }
  }
  pi[PH_MAXIT] = d->iterations;
  pi[PH_OFF_TAIL] = (int)pd.size();
  pd.resize(pd.size() + IT_SIZE);
  double *t = pd.data() + pi[PH_OFF_TAIL];
  for (int k = 0; k < 3; k++) { t[IT_SITE_POS + k] = d->site_pos[k]; t[IT_TGT_POS + k] = d->target_pos[k]; }
  for (int k = 0; k < 4; k++) { t[IT_SITE_QUAT + k] = d->site_quat[k]; t[IT_TGT_QUAT + k] = d->target_quat[k]; }
  t[IT_POS_TOL] = d->pos_tolerance;
  t[IT_ORI_TOL] = d->ori_tolerance;
  t[IT_DAMP] = d->damping > 0 ? d->damping : 1e-6;
  t[IT_LM] = d->lm_damping >= 0 ? d->lm_damping : 0.1;
  t[IT_MAX_STEP] = d->max_step > 0 ? d->max_step : 0.2;
  pi[PH_OFF_JRANGE] = (int)pd.size();
  for (int k = 0; k < 2 * m.njnt; k++) pd.push_back(d->jnt_range[k]);
  for (int k = 0; k < m.njnt; k++) pd.push_back(d->movable[k] ? 1.0 : 0.0);
  const size_t lds = (size_t)kPoseBlock * sizeof(double) * ((size_t)m.nq + 7 * (size_t)nj);  // + the step row
  if (lds > 64 * 1024) return fail(MJPL_E_CAPACITY, "IK: %d qpos + %d chain joints exceed the LDS budget", m.nq, nj);
  HIP_TRY(hipSetDevice(e->device));
  KtScope kt_scope(e, 1);  // (option "kernel_timer")
  // the program is tiny and changes with every target: staged through the engine's scratch
  const size_t ib = pi.size() * sizeof(int), db = pd.size() * sizeof(double);
  if ((rc = e->stage_ik.reserve(((ib + 7) & ~(size_t)7) + db, kStageFloor)) != MJPL_OK) return rc;
  int *d_pi = (int *)e->stage_ik.p;
  double *d_pd = (double *)(e->stage_ik.p + ((ib + 7) & ~(size_t)7));
  HIP_TRY(hipStreamSynchronize(e->stream));  // pageable host vectors go out of scope on return
  HIP_TRY(hipMemcpy(d_pi, pi.data(), ib, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_pd, pd.data(), db, hipMemcpyHostToDevice));
  const unsigned grid = (unsigned)((N + kPoseBlock - 1) / kPoseBlock);
  if (spec_k >= 0) {
    const RowsShape rs = rows_shape(N, e->rows_g);
    const int rc2 = e->spec->ik_solve(spec_k, rs.G, e->stream, rs.grid, d_pi, d_pd, dQ, N, rs.per, dQout, dok, diters, derr,
                                      d->restarts > 0 ? d->restarts : 0, (unsigned long long)d->restart_seed);
    if (rc2 == 0) return MJPL_OK;
    if (rc2 != -1) return fail(MJPL_E_HIP, "generated IK kernel failed to launch");
  }
  hipLaunchKernelGGL(k_ik_solve, dim3(grid), dim3(kPoseBlock), lds, e->stream, d_pi, d_pd, dQ, N, dQout, dok,
                     diters, derr, d->restarts > 0 ? d->restarts : 0, (uint64_t)d->restart_seed);
  HIP_TRY(hipGetLastError());
  return MJPL_OK;
}

int mjpl_ik_solve(mjpl_engine *e, const mjpl_ik_desc *d, const double *Q, int64_t N, double *Q_out,
                  uint8_t *ok, int32_t *iters, double *err) {
  if (!e || !d) return fail(MJPL_E_ARG, "mjpl_ik_solve: NULL argument");
  if (N < 0) return fail(MJPL_E_ARG, "negative batch size");
  if (N == 0) return MJPL_OK;
  if (!Q || !Q_out || !ok) return fail(MJPL_E_ARG, "NULL pointer");
  const size_t n = N, qb = n * e->m.nq * sizeof(double);
  const HostOut outs[] = {{Q_out, qb}, {ok, n}, {iters, n * sizeof(int32_t)}, {err, n * 2 * sizeof(double)}};
  return staged(e, false, {{Q, qb}}, outs, [&](void **in, void **out) {
    return mjpl_ik_solve_dev(e, d, (const double *)in[0], N, (double *)out[0], (uint8_t *)out[1], (int32_t *)out[2],
                             (double *)out[3]);
  });
}

}  // extern "C"

#include "mjpl_rrt.h"
