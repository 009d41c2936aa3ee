// Arguments of the two band launches of a nudged-elastic-band step (ta_neb.hip), filled by ta_relax_run
// (ta_api_relax.hip) in band mode (ta_relax_set_band). They run between the evaluation and the two FIRE launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ta {

struct NebLaunch {
  const double *pos;       // [F][n][3] db.pos: image after image, the same atoms in the same order
  const double *forces;    // [F][n][3] of the evaluation before this step
  const double *energy;    // [F] image energies of the same evaluation
  const uint8_t *fixed;    // [F][n] != 0: the atom's force is read as 0 and its band force is 0
  double *part;            // [(F - 2) blk_per_image][4]: t.t, F.t, d+.d+, d-.d- of the workgroup's atoms
  double *band;            // [F][n][3] band forces B; the rows of images 0 and F - 1 are never written (0)
  double *tau;             // [F][n][3] unit tangents, or null: not asked for by this launch
  int32_t *climbing;       // device word: the climbing image of this launch, -1 without climb
  const unsigned *status;  // as RelaxLaunch: 0, or 1 + seq of the launch whose drift left the list stale
  double k;                // spring constant, eV / A^2
  unsigned seq;            // steps of this run before this launch
  int n_images, n, chunk, blk_per_image;
  int climb;
};

// neb_reduce_kernel and neb_apply_kernel of one band step, in this order on `s`
void launch_neb_force(const NebLaunch &a, hipStream_t s);

}  // namespace ta
