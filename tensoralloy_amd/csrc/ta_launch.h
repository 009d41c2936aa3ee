// Host entry points of the model translation units (ta_mlp, ta_td, ta_train, ta_td_train, ta_hvp, ta_grap,
// ta_eam .hip) that other units call. The angular, list, MD, relaxation and band launchers are declared in
// ta_device.h, ta_md.h, ta_relax.h and ta_neb.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "ta_device.h"
#include "tensoralloy_amd.h"

namespace ta {
// per-atom networks (ta_mlp.hip, ta_td.hip)
size_t mlp_scratch_doubles(const MlpDev &mlp);
void launch_mlp_impl(const MlpDev &mlp, int activation, int ndim, const int32_t *atoms, int n_atoms,
                     const DeviceBatch &b, const Options &opt, double *scratch, hipStream_t s,
                     MlpLaunchInfo *info = nullptr, bool identity_atoms = false);
size_t mlp_all_scratch_doubles(const MlpDev *mlps_host, int nel, const int32_t *elem_start);
size_t td_scratch_doubles(const MlpDev *nets, int nel, int K, const int32_t *elem_start, bool da_global);
void launch_td_all(const MlpDev *nets_dev, const MlpDev *nets_host, int nel, int K, int act_h, int act,
                   int sommerfeld, int ndim, const DeviceBatch &b, bool da_global, const double *T, double *u_atom,
                   double *s_atom, double *scratch, hipStream_t s, MlpLaunchInfo *info = nullptr);
void launch_mlp_all(const MlpDev *mlps_dev, const MlpDev *mlps_host, int nel, int activation, int ndim,
                    const DeviceBatch &b, const Options &opt, double *scratch, hipStream_t s,
                    MlpLaunchInfo *info = nullptr);
// weight gradients (ta_train.hip)
int mlp_param_count(const MlpDev &mlp);
size_t mlp_grad_scratch_doubles(const MlpDev &mlp, int n_atoms);
size_t mlp_grad_partial_doubles(const MlpDev &mlp, int n_atoms);
void launch_mlp_grad(const MlpDev &mlp, int activation, int ndim, const int32_t *atoms, int n_atoms,
                     const DeviceBatch &b, const double *frame_coeff, double *scratch, double *partial,
                     double *grad, hipStream_t s);
void launch_mlp_grad_rows(const MlpDev &mlp, int activation, const int32_t *atoms, int n_rows,
                          const double *x, const double *row_coeff, const int32_t *frame_of_atom,
                          const double *frame_coeff, double *scratch, double *partial, double *grad,
                          hipStream_t s);
size_t mlp_grad2_scratch_doubles(const MlpDev &mlp, int n_atoms);
void launch_mlp_grad2(const MlpDev &mlp, int activation, int ndim, const int32_t *atoms, int n_atoms,
                      const DeviceBatch &b, const double *dG, const double *frame_coeff, double *scratch,
                      double *partial, double *grad, hipStream_t s, double *kappa_out = nullptr);
void launch_mlp_grad2_rows(const MlpDev &mlp, int activation, const int32_t *atoms, int n_rows, const double *x,
                           const double *xdot, const double *row_coeff, const int32_t *frame_of_atom,
                           const double *frame_coeff, double *scratch, double *partial, double *grad,
                           hipStream_t s);
void launch_grad_reduce(const double *partial, int n_blocks, int n_params, double *grad, hipStream_t s);
// weight gradients of the temperature-dependent head (ta_td_train.hip)
int td_param_count(const MlpDev *nets, int nel);
void td_grad2_sizes(const MlpDev *nets, int nel, int K, const int32_t *elem_start, size_t *scratch,
                    size_t *partial);
void launch_td_grad2(const MlpDev *nets_dev, const MlpDev *nets_host, int nel, int K, int act_h, int act,
                     int sommerfeld, int ndim, const DeviceBatch &b, const double *T, const double *dG,
                     const double *coeff, double *scratch, double *partial, double *grad, hipStream_t s);
// analytic Hessian-vector products of the descriptor models (ta_hvp.hip)
void launch_pair_vec(const DeviceBatch &b, double *Dv, hipStream_t s);
void launch_backward_hvp(const SFParams &sf, const AngChunk &ch, int nb, int ng, int nz, bool first, bool angular,
                         const DeviceBatch &b, const double *Dv, const double *Dd, const double *wdot, double *gv,
                         double *gd, hipStream_t s);
void launch_hvp_gather(const DeviceBatch &b, const double *Dv, const double *Dd, const double *gv, const double *gd,
                       double *fdot, double *wdot_at, hipStream_t s);
void launch_pair_tangent(const DeviceBatch &b, const double *dR, const double *dh, double *dD, hipStream_t s);
void launch_descriptor_jvp(const DeviceBatch &b, int ndim, const double *J, const double *dD, double *dG,
                           hipStream_t s);
void launch_one_hot(double *dEdG, int64_t n_atoms, int ndim, int c, hipStream_t s);
// GRAP (ta_grap.hip)
struct GrapModel;
bool grap_hvp_supported(const GrapModel *);
void launch_grap_hvp(GrapModel *, const DeviceBatch &b, double eps, const double *Dv, const double *Dd,
                     const double *wdot, double *gv, double *gd, hipStream_t s);
GrapModel *grap_create(const ta_model_desc *m, std::string &err);
int grap_ndim(const GrapModel *g);
bool grap_uses_filter_net(const GrapModel *g);
void grap_destroy(GrapModel *);
void grap_ensure(GrapModel *, const DeviceBatch &b);
void launch_grap_forward(GrapModel *, const DeviceBatch &b, double eps, hipStream_t s);
void launch_grap_backward(GrapModel *, const DeviceBatch &b, hipStream_t s);
// training the GRAP filter network (ta_grap.hip)
int64_t grap_filter_param_count(const GrapModel *g);
void grap_update_filter_weights(GrapModel *g, const double *flat, int64_t n, hipStream_t s);
int grap_filter_table_knots(const GrapModel *g);
void grap_set_filter_tables(GrapModel *g, bool on, int n_knots, hipStream_t s);
int grap_filter_table_target(const GrapModel *g, bool on, int n_knots);
void grap_mark_trained(GrapModel *g);
void grap_suspend_filter_tables(GrapModel *g, bool suspend);
std::string grap_filter_train_refusal(const GrapModel *g);
size_t grap_filter_grad_doubles(const GrapModel *g, const DeviceBatch &b);
void launch_grap_filter_tangent(GrapModel *g, const DeviceBatch &b, double eps, const double *Dv, const double *Dd,
                                double *Gdot, hipStream_t s);
void grap_filter_gradient(GrapModel *g, const DeviceBatch &b, double eps, const double *Dv, const double *Dd,
                          const double *kappa, double *scratch, double *grad, hipStream_t s);
// EAM / ADP (ta_eam.hip)
struct EamModel;
EamModel *eam_create(const ta_model_desc *m, const Options &opt, std::string &err);
void eam_destroy(EamModel *);
void eam_ensure(EamModel *, const DeviceBatch &b);
void eam_tabulate(EamModel *m, int n_r, const double *r, int n_rho, const double *rho, double *rho_of_r,
                  double *phi_of_r, double *embed_of_rho, double *u_of_r, double *w_of_r,
                  hipStream_t s);
void eam_compute(EamModel *, const DeviceBatch &b, uint32_t want, hipStream_t s,
                 hipEvent_t *ev /* 2 events or null */);
void eam_set_list_cutoff(EamModel *, double rc /* 0: the list is exact, no test */);
bool eam_is_plain(const EamModel *);
// on: forces go through eam_pair_kernel and the force gather (the route of the nn pair functions) for every model,
// so that an evaluation leaves the pair records and g[p] = the centre's terms of dE/dD; off (the default): analytic
// and tabulated pair functions take the one-pass force kernels
void eam_set_pair_route(EamModel *, bool on);
void eam_set_nn_tables(EamModel *, bool on);
bool eam_hvp_supported(const EamModel *);
size_t eam_hvp_extra_doubles(const EamModel *, const DeviceBatch &b, int n_dir);
void eam_hvp(EamModel *, const DeviceBatch &b, int n_dir, bool unit, int first, const double *dR, const double *dh,
             double *dFdot, double *fdot, double *wdot, double *extra, hipStream_t s);
bool eam_nn_tables_on(const EamModel *);
void eam_mark_trained(EamModel *);
int64_t eam_param_count(const EamModel *);
void eam_update_weights(EamModel *, const double *flat, int64_t n);
int64_t eam_constant_count(const EamModel *);
void eam_get_constants(const EamModel *, double *flat);
void eam_update_constants(EamModel *, const double *flat, int64_t n);
void eam_constant_gradient(EamModel *, const DeviceBatch &b, const double *frame_coeff, const double *dR,
                           const double *dh, double *grad, hipStream_t s);
void eam_energy_gradient(EamModel *, const DeviceBatch &b, const double *frame_coeff, double *grad,
                         hipStream_t s);
bool eam_loss_gradient_supported(const EamModel *);
void eam_loss_gradient(EamModel *, const DeviceBatch &b, const double *frame_coeff, const double *dR,
                       const double *dh, double *grad, hipStream_t s);
}  // namespace ta
