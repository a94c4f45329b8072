/*
 * multimesh_params.h -- an EXTENSION of the C ABI of multi_mesh_hip.so (multimesh_hip.h): conversion of models and of
 * sensitivity kernels between seismic parametrisations, per node, on arrays that stay in HBM.  The two entry points live in
 * the same library; they are declared here and not in multimesh_hip.h because that header's set of functions is pinned by the
 * binding tests ("Parametrisations").  Bound by multimesh_amd/parametrisation.py.
 *
 * PARAMETRISATIONS, numbered in this order, with their components in this order:
 *   0 iso_velocity   VP, VS, RHO
 *   1 iso_lame       LAMBDA, MU, RHO
 *   2 iso_bulk       KAPPA, MU, RHO
 *   3 vti_velocity   VPV, VPH, VSV, VSH, ETA, RHO
 *   4 vti_love       A, C, L, N, F, RHO
 *
 * STEPS.  Eight directed steps, one ring: iso_velocity -- iso_lame -- iso_bulk <- vti_love -- vti_velocity <- iso_velocity
 * (steps 7 and 8 go one way only).  A conversion from -> to is the legal route with the fewest steps (never a tie), the
 * composition of its steps' statements; RHO is copied by every step.  THE STATEMENT, every operation an IEEE-754 binary64
 * operation rounded on its own, sums left to right as written, x * x for a square, no fused multiply-add:
 *   1 iso_velocity -> iso_lame     MU = RHO * (VS * VS);  LAMBDA = RHO * (VP * VP) - 2.0 * MU
 *   2 iso_lame -> iso_velocity     VS = sqrt(MU / RHO);   VP = sqrt((LAMBDA + 2.0 * MU) / RHO)
 *   3 iso_lame -> iso_bulk         KAPPA = LAMBDA + (2.0 * MU) / 3.0
 *   4 iso_bulk -> iso_lame         LAMBDA = KAPPA - (2.0 * MU) / 3.0
 *   5 vti_velocity -> vti_love     A = RHO * (VPH * VPH);  C = RHO * (VPV * VPV);  L = RHO * (VSV * VSV);
 *                                  N = RHO * (VSH * VSH);  F = ETA * (A - 2.0 * L)
 *   6 vti_love -> vti_velocity     VPV = sqrt(C / RHO);  VPH = sqrt(A / RHO);  VSV = sqrt(L / RHO);  VSH = sqrt(N / RHO);
 *                                  ETA = F / (A - 2.0 * L)
 *   7 iso_velocity -> vti_velocity VPV = VPH = VP;  VSV = VSH = VS;  ETA = 1.0  (copies of the bits, no arithmetic)
 *   8 vti_love -> iso_bulk         KAPPA = (((C + 4.0 * A) - 4.0 * N) + 4.0 * F) / 9.0;
 *                                  MU = ((((A + C) + 6.0 * L) + 5.0 * N) - 2.0 * F) / 15.0   (the Voigt average)
 * Nothing is special-cased: VS = 0, RHO = 0, A - 2 L = 0, a negative argument of sqrt, NaN, +-inf, -0.0 and denormals give
 * what IEEE arithmetic gives (the payload and sign of a NaN that an operation produces are the processor's).
 *
 * THE TRANSPOSED JACOBIANS (mm_convert_kernels).  With m the INPUT of a step and K' the kernel with respect to its outputs,
 * K = J^T K' with respect to its inputs; r2 = 2.0 * RHO; sums left to right as written:
 *   1  K_VP = (r2 * VP) * K'_LAMBDA;  K_VS = (r2 * VS) * (K'_MU - 2.0 * K'_LAMBDA);
 *      K_RHO = (K'_RHO + (VP * VP - 2.0 * (VS * VS)) * K'_LAMBDA) + (VS * VS) * K'_MU
 *   2  with VS, VP of the statement:  K_LAMBDA = K'_VP / (r2 * VP);  K_MU = K'_VP / (RHO * VP) + K'_VS / (r2 * VS);
 *      K_RHO = (K'_RHO - (VP / r2) * K'_VP) - (VS / r2) * K'_VS
 *   3  K_LAMBDA = K'_KAPPA;  K_MU = K'_MU + (2.0 * K'_KAPPA) / 3.0;  K_RHO = K'_RHO
 *   4  K_KAPPA = K'_LAMBDA;  K_MU = K'_MU - (2.0 * K'_LAMBDA) / 3.0;  K_RHO = K'_RHO
 *   5  with A, L of the statement, a = K'_A + ETA * K'_F, l = K'_L - 2.0 * (ETA * K'_F):
 *      K_VPV = (r2 * VPV) * K'_C;  K_VPH = (r2 * VPH) * a;  K_VSV = (r2 * VSV) * l;  K_VSH = (r2 * VSH) * K'_N;
 *      K_ETA = (A - 2.0 * L) * K'_F;
 *      K_RHO = (((K'_RHO + (VPH * VPH) * a) + (VPV * VPV) * K'_C) + (VSV * VSV) * l) + (VSH * VSH) * K'_N
 *   6  with the velocities and ETA of the statement, d = A - 2.0 * L, g = ETA / d:
 *      K_A = K'_VPH / (r2 * VPH) - g * K'_ETA;  K_C = K'_VPV / (r2 * VPV);  K_L = K'_VSV / (r2 * VSV) + (2.0 * g) * K'_ETA;
 *      K_N = K'_VSH / (r2 * VSH);  K_F = K'_ETA / d;
 *      K_RHO = (((K'_RHO - (VPV / r2) * K'_VPV) - (VPH / r2) * K'_VPH) - (VSV / r2) * K'_VSV) - (VSH / r2) * K'_VSH
 *   7  K_VP = K'_VPV + K'_VPH;  K_VS = K'_VSV + K'_VSH;  K_RHO = K'_RHO   (K'_ETA does not enter)
 *   8  with a = K'_KAPPA / 9.0, b = K'_MU / 15.0:
 *      K_A = 4.0 * a + b;  K_C = a + b;  K_L = 6.0 * b;  K_N = 5.0 * b - 4.0 * a;  K_F = 4.0 * a - 2.0 * b;  K_RHO = K'_RHO
 * A route's transform runs the route forward, keeping every step's input, and applies the steps' transposes in reverse order.
 * Kernels are ABSOLUTE (dchi/dp); relative kernels (p * dchi/dp) are not converted.
 *
 * ADDRESSING.  Component c of node p of group e of an array is base[e * group_stride + cols[c] * comp_stride + p], in
 * elements, 0 <= p < P, 0 <= e < ngroups.  Field planes [C][E][P]: group_stride = P, comp_stride = E * P, cols = 0, 1, ...;
 * MODEL/data [E][C_total][P]: group_stride = C_total * P, comp_stride = P, cols = the parametrisation's columns.  cols are
 * HOST arrays with one entry per component of the array's parametrisation (3 or 6), copied into the kernel's arguments.
 *
 * Both entry points run on the context's stream and do not synchronise.  nbad_d: int64[1] ON THE DEVICE, or NULL: the number of
 * nodes with at least one output that is not finite is ADDED to it (integer atomics: the same on every run); it is not zeroed.
 * The output may be an input array with the same strides (every lane reads all of its node's inputs before it writes, and
 * touches no other node); otherwise it may share no byte with an input.
 * MM_ERR_ARG, decided on the host before the device is touched and with nothing written, for a null ctx, array or cols (an
 * array may be null when ngroups == 0); from or to outside 0..4, or from == to; a negative ngroups; P outside [1, 4096]; a
 * negative column or stride; two equal output columns; an output layout in which two nodes or components share an element;
 * an array whose extent (ngroups - 1) * group_stride + max(cols) * comp_stride + P is at or past 2^48 elements; an output that
 * overlaps an input without being that array with its strides.  ngroups == 0 is valid.
 */
#ifndef MULTIMESH_PARAMS_H
#define MULTIMESH_PARAMS_H

#include "multimesh_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_PARAM_ISO_VELOCITY 0
#define MM_PARAM_ISO_LAME 1
#define MM_PARAM_ISO_BULK 2
#define MM_PARAM_VTI_VELOCITY 3
#define MM_PARAM_VTI_LOVE 4
#define MM_PARAM_MAX_COMPONENTS 6
#define MM_PARAM_MAX_P 4096

/* out (parametrisation `to`) = the route's statement applied to in (parametrisation `from`), node by node. */
int mm_convert_parameters(mm_context *ctx, int from, int to, int64_t ngroups, int64_t P,
                          const double *in_d, int64_t in_group_stride, int64_t in_comp_stride, const int *in_cols,
                          double *out_d, int64_t out_group_stride, int64_t out_comp_stride, const int *out_cols,
                          int64_t *nbad_d);

/* kout (with respect to `from`) = J^T kin (with respect to `to`), J = d to / d from at the model (in `from`), node by node.
 * model_cols and kout_cols have the components of `from`, kin_cols those of `to`. */
int mm_convert_kernels(mm_context *ctx, int from, int to, int64_t ngroups, int64_t P,
                       const double *model_d, int64_t model_group_stride, int64_t model_comp_stride, const int *model_cols,
                       const double *kin_d, int64_t kin_group_stride, int64_t kin_comp_stride, const int *kin_cols,
                       double *kout_d, int64_t kout_group_stride, int64_t kout_comp_stride, const int *kout_cols,
                       int64_t *nbad_d);

#ifdef __cplusplus
}
#endif
#endif /* MULTIMESH_PARAMS_H */
