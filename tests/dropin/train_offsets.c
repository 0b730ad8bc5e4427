/* train_offsets.c -- offsetof / sizeof of every field of optimizer_adam (SRC/optimizer/adam.h:16-42) and
 * nfft4gp_gp_problem (SRC/optimizer/gp_problem.h:20-74), and the optimizer enum's values.  Compiled twice by
 * tests/test_train_host.py: once against the reference's own headers (-DUSE_REF) and once against
 * include/nfft4gp_amd.h; the two outputs must be identical. */
#include <stddef.h>
#include <stdio.h>
#ifdef USE_REF
#include "adam.h"       /* SRC/optimizer */
#include "gp_problem.h" /* SRC/optimizer */
#else
#include "nfft4gp_amd.h"
#endif

#define F(T, f) printf("%s.%s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))
int main(void)
{
   printf("optimizer_adam %zu\n", sizeof(optimizer_adam));
   F(optimizer_adam, _maxits);
   F(optimizer_adam, _tol);
   F(optimizer_adam, _floss);
   F(optimizer_adam, _fdata);
   F(optimizer_adam, _n);
   F(optimizer_adam, _beta1);
   F(optimizer_adam, _beta2);
   F(optimizer_adam, _epsilon);
   F(optimizer_adam, _alpha);
   F(optimizer_adam, _m);
   F(optimizer_adam, _v);
   F(optimizer_adam, _m_hat);
   F(optimizer_adam, _v_hat);
   F(optimizer_adam, _nits);
   F(optimizer_adam, _loss_history);
   F(optimizer_adam, _x_history);
   F(optimizer_adam, _grad_history);
   F(optimizer_adam, _grad_norm_history);
   printf("nfft4gp_gp_problem %zu\n", sizeof(nfft4gp_gp_problem));
   F(nfft4gp_gp_problem, _type);
   F(nfft4gp_gp_problem, _fstep);
   F(nfft4gp_gp_problem, _optimizer);
   F(nfft4gp_gp_problem, _dwork);
   F(nfft4gp_gp_problem, _data_train);
   F(nfft4gp_gp_problem, _data_train_n);
   F(nfft4gp_gp_problem, _data_train_ldim);
   F(nfft4gp_gp_problem, _data_train_d);
   F(nfft4gp_gp_problem, _label_train);
   F(nfft4gp_gp_problem, _fkernel);
   F(nfft4gp_gp_problem, _vfkernel_data);
   F(nfft4gp_gp_problem, _kernel_data_free);
   F(nfft4gp_gp_problem, _matvec);
   F(nfft4gp_gp_problem, _dmatvec);
   F(nfft4gp_gp_problem, _precond_fkernel);
   F(nfft4gp_gp_problem, _precond_vfkernel_data);
   F(nfft4gp_gp_problem, _precond_kernel_data_free);
   F(nfft4gp_gp_problem, _precond_setup);
   F(nfft4gp_gp_problem, _precond_solve);
   F(nfft4gp_gp_problem, _precond_trace);
   F(nfft4gp_gp_problem, _precond_logdet);
   F(nfft4gp_gp_problem, _precond_dvp);
   F(nfft4gp_gp_problem, _precond_reset);
   F(nfft4gp_gp_problem, _precond_data);
   F(nfft4gp_gp_problem, _atol_loss);
   F(nfft4gp_gp_problem, _tol_loss);
   F(nfft4gp_gp_problem, _wsize_loss);
   F(nfft4gp_gp_problem, _maxits_loss);
   F(nfft4gp_gp_problem, _nvecs_loss);
   F(nfft4gp_gp_problem, _radamacher_loss);
   F(nfft4gp_gp_problem, _transform);
   F(nfft4gp_gp_problem, _mask);
   F(nfft4gp_gp_problem, _print_level_loss);
   F(nfft4gp_gp_problem, _data_predict);
   F(nfft4gp_gp_problem, _data_predict_n);
   F(nfft4gp_gp_problem, _data_predict_ldim);
   F(nfft4gp_gp_problem, _data_predict_d);
   F(nfft4gp_gp_problem, _label_predict);
   F(nfft4gp_gp_problem, _matvec_predict);
   F(nfft4gp_gp_problem, _atol_predict);
   F(nfft4gp_gp_problem, _tol_predict);
   F(nfft4gp_gp_problem, _wsize_predict);
   F(nfft4gp_gp_problem, _maxits_predict);
   F(nfft4gp_gp_problem, _print_level_predict);
   F(nfft4gp_gp_problem, _retuire_std);
   printf("optimizer enum %d %d %d %zu\n", (int)NFFT4GP_OPTIMIZER_UNDEFINED, (int)NFFT4GP_OPTIMIZER_ADAM,
          (int)NFFT4GP_OPTIMIZER_NLTGCR, sizeof(nfft4gp_optimizer_type));
   printf("func types %zu %zu %zu\n", sizeof(func_loss), sizeof(func_optimization_step), sizeof(func_matvec));
   return 0;
}
