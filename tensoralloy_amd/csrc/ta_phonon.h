// Launches of the harmonic-phonon path (ta_phonon.hip), filled by the ta_phonon_* entry points (ta_api_phonon.hip).
// Complex arrays are interleaved (re, im) doubles. Matrices are row-major.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tensoralloy_amd.h"

namespace ta {

constexpr int kPhononMaxOrder = TA_PHONON_MAX_ORDER;  // the solver's largest matrix
constexpr int kPhononSweepCap = 40;                   // cyclic Jacobi sweeps before a matrix counts as unconverged
constexpr int kPhononDosSlab = 64;                    // q-points per workgroup of the DOS launch (see ta_phonon.hip)

struct PhononDynmatLaunch {
  const double *phi;         // [n_basis][N][3][3] force constants of the home-cell atoms
  const int32_t *basis_of;   // [N] home-cell atom every supercell atom is an image of
  const double *mass;        // [n_basis] amu
  const int32_t *start;      // [n_basis N + 1] CSR offsets into vec, pair (b, s) at b N + s
  const double *vec;         // [n_vec][3] shortest vectors b -> images of s, Angstrom
  const double *q;           // [Q][3] Cartesian, 1 / Angstrom
  double *D;                 // [Q][n][n] complex
  int n_basis, N;
  long long Q;
};

struct PhononEighLaunch {
  const double *A;           // [batch][n][n] complex; the Hermitian part (A + A^H) / 2 is what is solved
  double *w;                 // [batch][n] ascending
  double *V;                 // [batch][n][n] complex or null: row m = eigenvector m
  unsigned long long *info;  // += matrices that reached the sweep cap
  int n;
  long long batch;
};

struct PhononDosLaunch {
  const double *w;            // [Q][n] eigenvalues of the chunk
  const double *V;            // [Q][n][n] complex or null (total only)
  unsigned long long *total;  // [n_bins]
  unsigned long long *info;   // += modes outside [nu_min, nu_max)
  double *slab_part;          // [slabs][n_basis][n_bins] zeroed by the launch, or null
  double *partial;            // [n_basis][n_bins] running sums, slabs added in index order
  double nu_min, inv_dnu, factor;
  int n, n_bins;
  long long Q;
};

// matrices one workgroup of the solver takes, and its dynamic LDS bytes, for order n (with eigenvectors or not)
int phonon_eigh_matrices_per_block(int n);
void launch_phonon_dynmat(const PhononDynmatLaunch &a, hipStream_t s);
void launch_phonon_eigh(const PhononEighLaunch &a, hipStream_t s);
// nu[i] = sign(w[i]) sqrt(|w[i]|) factor
void launch_phonon_frequencies(const double *w, double *nu, long long n, double factor, hipStream_t s);
void launch_phonon_dos(const PhononDosLaunch &a, hipStream_t s);
// phi[b][s][a][c] = -raw[3 b + a][3 s + c]   (raw: the force tangents of 3 n_basis unit displacements)
void launch_phonon_phi_from_tangents(const double *raw, double *phi, int n_basis, int N, hipStream_t s);

}  // namespace ta
