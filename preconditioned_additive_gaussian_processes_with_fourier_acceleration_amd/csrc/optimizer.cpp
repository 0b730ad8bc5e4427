// optimizer.cpp -- the training loop under the reference's names: the Adam optimiser (SRC/optimizer/adam.c) and
// the GP problem that carries Nfft4GPGpLoss's arguments (SRC/optimizer/gp_problem.c).  Host code: an Adam step
// is a handful of flops on three hyperparameters; all the work is in the loss it calls.
//
// Semantics kept from the reference: the histories hold maxits + 1 entries with the starting point in entry 0;
// SetOptions and Init refuse once a step has been taken; Step returns 0 / 1 (maxits) / 2 (gradient norm below
// tol) / -1 (loss failed, _nits untouched); the banner and the per-step line have the reference's format.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/nfft4gp_amd.h"

namespace {

double* zeros(size_t count) { return (double*)calloc(count ? count : 1, sizeof(double)); }

void release(double*& p)
{
   free(p);
   p = nullptr;
}

}  // namespace

extern "C" {

void* Nfft4GPOptimizationAdamCreate(void)
{
   optimizer_adam* A = (optimizer_adam*)calloc(1, sizeof(optimizer_adam));  // pointers NULL, counters 0
   if (!A) return NULL;
   A->_maxits = 1000;
   A->_tol = 1e-6;
   A->_beta1 = 0.9;
   A->_beta2 = 0.999;
   A->_epsilon = 1e-8;
   A->_alpha = 0.001;
   return A;
}

void Nfft4GPOptimizationAdamFree(void* optimizer)
{
   optimizer_adam* A = (optimizer_adam*)optimizer;
   if (!A) return;
   release(A->_m);
   release(A->_v);
   release(A->_m_hat);
   release(A->_v_hat);
   release(A->_loss_history);
   release(A->_x_history);
   release(A->_grad_history);
   release(A->_grad_norm_history);
   free(A);
}

int Nfft4GPOptimizationAdamSetProblem(void* optimizer, func_loss floss, void* fdata, int n)
{
   optimizer_adam* A = (optimizer_adam*)optimizer;
   A->_floss = floss;
   A->_fdata = fdata;
   A->_n = n;
   return 0;
}

int Nfft4GPOptimizationAdamSetOptions(void* optimizer, int maxits, double tol, double beta1, double beta2,
                                      double epsilon, double alpha)
{
   optimizer_adam* A = (optimizer_adam*)optimizer;
   if (A->_nits > 0) {
      printf("Error: cannot set options after the first optimization step.\n");
      return -1;
   }
   A->_maxits = maxits;
   A->_tol = tol;
   A->_beta1 = beta1;
   A->_beta2 = beta2;
   A->_epsilon = epsilon;
   A->_alpha = alpha;
   return 0;
}

int Nfft4GPOptimizationAdamInit(void* optimizer, double* x)
{
   optimizer_adam* A = (optimizer_adam*)optimizer;
   if (A->_nits > 0) {
      printf("Error: cannot initialize after the first optimization step.\n");
      return -1;
   }
   const size_t n = (size_t)(A->_n > 0 ? A->_n : 0), len = (size_t)(A->_maxits > 0 ? A->_maxits : 0) + 1;
   // a second Init before any step starts over
   release(A->_m);
   release(A->_v);
   release(A->_m_hat);
   release(A->_v_hat);
   release(A->_loss_history);
   release(A->_x_history);
   release(A->_grad_history);
   release(A->_grad_norm_history);
   A->_m = zeros(n);
   A->_v = zeros(n);
   A->_m_hat = zeros(n);
   A->_v_hat = zeros(n);
   A->_loss_history = zeros(len);
   A->_x_history = zeros(len * n);
   A->_grad_history = zeros(len * n);
   A->_grad_norm_history = zeros(len);
   if (!A->_m || !A->_v || !A->_m_hat || !A->_v_hat || !A->_loss_history || !A->_x_history || !A->_grad_history ||
       !A->_grad_norm_history)
      return -1;
   memcpy(A->_x_history, x, sizeof(double) * n);
   printf("Iteration  | Loss            | Grad norm     \n");
   return 0;
}

int Nfft4GPOptimizationAdamStep(void* optimizer)
{
   optimizer_adam* A = (optimizer_adam*)optimizer;
   const int n = A->_n, it = A->_nits;
   if (!A->_floss || !A->_x_history) return -1;  // no problem set, or no Init
   if (it >= A->_maxits) return 1;               // the histories (maxits + 1 entries) are full
   double* x = A->_x_history + (size_t)it * n;
   double* g = A->_grad_history + (size_t)it * n;
   double* xn = A->_x_history + (size_t)(it + 1) * n;
   if (A->_floss(A->_fdata, x, A->_loss_history + it, g) != 0) {
      printf("Loss failed\n");
      printf("Current x:\n");
      for (int i = 0; i < n; i++) printf("%15.8e ", x[i]);
      printf("\n");
      return -1;
   }
   // bias corrections of step it + 1
   const double c1 = 1.0 - pow(A->_beta1, it + 1.0), c2 = 1.0 - pow(A->_beta2, it + 1.0);
   double gg = 0.0;
   for (int i = 0; i < n; i++) {
      A->_m[i] = A->_beta1 * A->_m[i] + (1.0 - A->_beta1) * g[i];
      A->_v[i] = A->_beta2 * A->_v[i] + (1.0 - A->_beta2) * g[i] * g[i];
      A->_m_hat[i] = A->_m[i] / c1;
      A->_v_hat[i] = A->_v[i] / c2;
      xn[i] = x[i] - A->_alpha * A->_m_hat[i] / (sqrt(A->_v_hat[i]) + A->_epsilon);
      gg += g[i] * g[i];
   }
   const double gnorm = sqrt(gg);
   A->_grad_norm_history[it] = gnorm;
   A->_nits = it + 1;

   // iteration | loss | gradient norm | the new parameters | the same after the softplus transform
   const int np = n < 3 ? n : 3;
   printf("%10d | %15.8e | %15.8e | current params: ", A->_nits, A->_loss_history[it], gnorm);
   for (int i = 0; i < np; i++) printf(i ? ", %15.8e" : "%15.8e", xn[i]);
   printf(" | current params (after transform): ");
   for (int i = 0; i < np; i++) {
      double t = 0.0, dt = 0.0;
      Nfft4GPTransform(NFFT4GP_TRANSFORM_SOFTPLUS, xn[i], 0, &t, &dt);
      printf(i ? ", %15.8e" : "%15.8e", t);
   }
   printf("\n");

   if (gnorm < A->_tol) {
      printf("Iteration stopped at %d with norm %e\n", A->_nits, gnorm);
      return 2;
   }
   return A->_nits >= A->_maxits ? 1 : 0;
}

void* Nfft4GPGPProblemCreate(void)
{
   nfft4gp_gp_problem* G = (nfft4gp_gp_problem*)calloc(1, sizeof(nfft4gp_gp_problem));
   if (!G) return NULL;
   // everything else NULL / 0 (NFFT4GP_OPTIMIZER_UNDEFINED, full re-orthogonalisation, no printing)
   G->_tol_loss = 1e-4;
   G->_maxits_loss = 50;
   G->_nvecs_loss = 5;
   G->_transform = NFFT4GP_TRANSFORM_SOFTPLUS;
   G->_tol_predict = 1e-6;
   G->_maxits_predict = 100;
   return G;
}

void Nfft4GPGPProblemFree(void* gp_problem)
{
   nfft4gp_gp_problem* G = (nfft4gp_gp_problem*)gp_problem;
   if (!G) return;
   free(G->_dwork);
   free(G);
}

int Nfft4GPGpProblemSetup(void* gp_problem, nfft4gp_optimizer_type type, func_optimization_step fstep, void* optimizer,
                          double* data_train, int data_train_n, int data_train_ldim, int data_train_d,
                          double* label_train, func_kernel fkernel, void* vfkernel_data, func_free kernel_data_free,
                          func_symmatvec matvec, func_symmatvec dmatvec, func_kernel precond_fkernel,
                          void* precond_vfkernel_data, func_free precond_kernel_data_free,
                          precond_kernel_setup precond_setup, func_solve precond_solve, func_trace precond_trace,
                          func_logdet precond_logdet, func_dvp precond_dvp, func_free precond_reset,
                          void* precond_data, int atol_loss, double tol_loss, int wsize_loss, int maxits_loss,
                          int nvecs_loss, double* radamacher_loss, nfft4gp_transform_type transform, int* mask,
                          int print_level_loss, double* data_predict, int data_predict_n, int data_predict_ldim,
                          int data_predict_d, double* label_predict, func_matvec matvec_predict, int atol_predict,
                          double tol_predict, int wsize_predict, int maxits_predict, int print_level_predict,
                          int retuire_std)
{
   if (!gp_problem) {
      printf("Error: gp_problem is NULL.\n");
      return -1;
   }
   nfft4gp_gp_problem* G = (nfft4gp_gp_problem*)gp_problem;
   G->_type = type;
   G->_fstep = fstep;
   G->_optimizer = optimizer;
   G->_data_train = data_train;
   G->_data_train_n = data_train_n;
   G->_data_train_ldim = data_train_ldim;
   G->_data_train_d = data_train_d;
   G->_label_train = label_train;
   G->_fkernel = fkernel;
   G->_vfkernel_data = vfkernel_data;
   G->_kernel_data_free = kernel_data_free;
   G->_matvec = matvec;
   G->_dmatvec = dmatvec;
   G->_precond_fkernel = precond_fkernel;
   G->_precond_vfkernel_data = precond_vfkernel_data;
   G->_precond_kernel_data_free = precond_kernel_data_free;
   G->_precond_setup = precond_setup;
   G->_precond_solve = precond_solve;
   G->_precond_trace = precond_trace;
   G->_precond_logdet = precond_logdet;
   G->_precond_dvp = precond_dvp;
   G->_precond_reset = precond_reset;
   G->_precond_data = precond_data;
   G->_atol_loss = atol_loss;
   G->_tol_loss = tol_loss;
   G->_wsize_loss = wsize_loss;
   G->_maxits_loss = maxits_loss;
   G->_nvecs_loss = nvecs_loss;
   G->_radamacher_loss = radamacher_loss;
   G->_transform = transform;
   G->_mask = mask;
   G->_print_level_loss = print_level_loss;
   G->_data_predict = data_predict;
   G->_data_predict_n = data_predict_n;
   G->_data_predict_ldim = data_predict_ldim;
   G->_data_predict_d = data_predict_d;
   G->_label_predict = label_predict;
   G->_matvec_predict = matvec_predict;
   G->_atol_predict = atol_predict;
   G->_tol_predict = tol_predict;
   G->_wsize_predict = wsize_predict;
   G->_maxits_predict = maxits_predict;
   G->_print_level_predict = print_level_predict;
   G->_retuire_std = retuire_std;
   return 0;
}

int Nfft4GPGpProblemLoss(void* problem, double* x, double* lossp, double* dloss)
{
   nfft4gp_gp_problem* G = (nfft4gp_gp_problem*)problem;
   if (!G) return -1;
   return Nfft4GPGpLoss(x, G->_data_train, G->_label_train, G->_data_train_n, G->_data_train_ldim, G->_data_train_d,
                        G->_fkernel, G->_vfkernel_data, G->_kernel_data_free, G->_matvec, G->_dmatvec,
                        G->_precond_fkernel, G->_precond_vfkernel_data, G->_precond_kernel_data_free,
                        G->_precond_setup, G->_precond_solve, G->_precond_trace, G->_precond_logdet, G->_precond_dvp,
                        G->_precond_reset, G->_precond_data, G->_atol_loss, G->_tol_loss, G->_wsize_loss,
                        G->_maxits_loss, G->_nvecs_loss, G->_radamacher_loss, G->_transform, G->_mask,
                        G->_print_level_loss, G->_dwork, lossp, dloss);
}

}  // extern "C"
