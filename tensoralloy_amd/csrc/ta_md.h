// Arguments of the MD integrator launch (ta_md.hip), filled by ta_md_run (ta_api.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ta {

constexpr int kMdChunk = 1024;      // atoms per workgroup without a thermostat (256 threads, 4 atoms each)
constexpr int kMdLookahead = 4;     // steps ta_md_run enqueues between two looks at the status word

struct MdLaunch {
  double *pos;                // [N][3] db.pos, caller's atom order
  double *vel;                // [N][3]
  const double *forces;       // [N][3] of the evaluation before this launch
  const double *mass;         // [N]
  const double *ref;          // [N][3] positions the resident list was built for
  const double *energy;       // [F] frame energies of the evaluation before this launch
  const int32_t *atom_start;  // [F + 1]
  const int32_t *blk_start;   // [F + 1] first workgroup of each frame
  double *epot;               // [n_rec][F]
  double *ke_part;            // [n_rec][n_blk]
  unsigned *status;           // device word: 0, or 1 + seq of the launch whose drift left the list stale
  unsigned *status_host;      // the same, page-locked
  double dt, kT0, dt_over_tau;
  double lim2;                // skin^2 / 4; negative: every drift is stale (skin = 0)
  long long rec;              // record slot, -1: none
  unsigned seq;               // steps of this run before this launch
  int n_frames, n_blk, chunk;
  int kick2;                  // the second half-kick is pending
  int drift;                  // 0: only finish the step (last launch of a run)
};

void launch_md_integrate(const MdLaunch &a, int threads, hipStream_t s);

}  // namespace ta
