// Arguments of the two launches of a FIRE step (ta_relax.hip), filled by ta_relax_run (ta_api_relax.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ta {

// FIRE state of one frame. Two copies per frame: launch k reads copy k & 1 and writes copy (k + 1) & 1.
struct RelaxFrameState {
  double dt, a;
  double fmax2;       // max_i |F_i|^2 of the last evaluation this frame was tested with
  int32_t npos;       // steps with F.v > 0 since the last reset
  int32_t first;      // no step taken since ta_relax_init: the velocities count as 0
  int32_t converged;  // frozen for the rest of the run
  int32_t steps;      // steps taken in this run
};

struct RelaxLaunch {
  double *pos;                // [N][3] db.pos, caller's atom order
  double *vel;                // [N][3] FIRE velocities (the relaxation's own array)
  const double *forces;       // [N][3] of the evaluation before this step
  const uint8_t *fixed;       // [N] != 0: the atom's force is read as 0 and it is never written
  const double *ref;          // [N][3] positions the resident list was built for
  const int32_t *atom_start;  // [F + 1]
  const int32_t *blk_start;   // [F + 1] first workgroup of each frame
  double *part;               // [n_blk][4]: F.v, F.F, v.v, max |F_i|^2 of the workgroup's atoms
  RelaxFrameState *state;     // [2][F]
  int *n_converged;           // device word: frames that converged in this run
  unsigned *status;           // as MdLaunch: 0, or 1 + seq of the launch whose drift left the list stale
  unsigned *status_host;      // [0] the same, page-locked; [1] 1 + seq of the launch at which the last frame converged
  double dtmax, maxstep, finc, fdec, astart, fa;
  double fmax2;               // a frame with max_i |F_i|^2 < fmax2 is converged
  double lim2;                // skin^2 / 4; negative: every drift is stale (skin = 0)
  unsigned seq;               // steps of this run before this launch
  int nmin, n_frames, n_blk, chunk;
  int drift;                  // 0: only the convergence test (last launch of a run that used up its steps)
  // cell mode only (ta_relax_set_cell; the launches' kCell builds): the rows [q_1 .. q_n ; cf G] are relaxed
  const double *virial;       // [F][9] W of the evaluation before this step
  double *cells;              // [F][9] db.cells: written by the frame's first workgroup, read by no workgroup
  const double *ref_cells;    // [F][9] cells the resident list was built for
  const double *cell_h0;      // [F][9] cells at ta_relax_set_cell
  const double *cell_cf;      // [F] cell factor
  double *cell_G;             // [2][F][9] deformation gradient, double-buffered as `state`
  double *cell_vel;           // [2][F][9] FIRE velocity of the rows cf G, likewise
  double *cell_fmax2;         // [F] max row |f_cell|^2 of the last evaluation the frame was tested with
  double cell_mask[9];        // 0 / 1, symmetric
  double pressure;            // eV / A^3
  double skin, r_list;        // r_list = max(rcut, acut) + skin
  int hydrostatic;
  int cell;                   // 0: the fixed-cell builds run and nothing above is read
};

// the reduce launch and the step launch of one FIRE step, in this order on `s`
void launch_relax_step(const RelaxLaunch &a, hipStream_t s);

}  // namespace ta
