// gp_loss.hip -- the GP negative log marginal likelihood with its gradient, the hyperparameter transforms, and
// the additive-kernel prediction, on the solvers of fgmres.hip and lanczos.hip.
//
//   Nfft4GPGpLoss                  SRC/optimizer/gp_loss.c:96-307
//   Nfft4GPTransform               SRC/optimizer/transform.c:4-89
//   Nfft4GPAdditiveNFFTGpPredict   SRC/external/nfft_interface.c:873-1068 (posterior mean, and the
//                                  predictive standard deviation by one solve per prediction point)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "krylov.hpp"

using namespace nfft4gp_amd;

namespace {

// E[s ld + r0 + s] = 1 (unit columns of the predict's K12 / K22 probes; E zeroed before)
__global__ void k_set_units(double* __restrict__ E, size_t ld, size_t r0, int m)
{
   const int s = blockIdx.x * blockDim.x + threadIdx.x;
   if (s < m) E[(size_t)s * ld + r0 + s] = 1.0;
}

// out[s] = Y[s ld + r0 + s]
__global__ void k_pick_diag(double* __restrict__ out, const double* __restrict__ Y, size_t ld, size_t r0, int m)
{
   const int s = blockIdx.x * blockDim.x + threadIdx.x;
   if (s < m) out[s] = Y[(size_t)s * ld + r0 + s];
}

}  // namespace

extern "C" {

int Nfft4GPTransform(nfft4gp_transform_type type, double val, int inverse, double* tvalp, double* dtvalp)
{
   switch (type) {
   case 1:  // NFFT4GP_TRANSFORM_SIGMOID
      if (!inverse) {
         *tvalp = 1.0 / (exp(-val) + 1.0);
         *dtvalp = *tvalp * (1 - *tvalp);
      } else {
         *tvalp = log(val / (1.0 - val));
      }
      break;
   case 0:  // NFFT4GP_TRANSFORM_SOFTPLUS
      if (!inverse) {
         if (val > 20.0) {
            *tvalp = val;
            *dtvalp = 1.0;
         } else if (val < -20.0) {
            *tvalp = exp(val);
            *dtvalp = exp(val);
         } else {
            *tvalp = log(1.0 + exp(val));
            *dtvalp = exp(val) / (1.0 + exp(val));
         }
      } else {
         if (val > 20.0)
            *tvalp = val;
         else if (val < 2.06115362243856e-09)
            *tvalp = log(val);
         else
            *tvalp = log(exp(val) - 1.0);
      }
      break;
   case 2:  // NFFT4GP_TRANSFORM_EXP
      if (!inverse) {
         *tvalp = exp(val);
         *dtvalp = exp(val);
      } else {
         *tvalp = log(val);
      }
      break;
   case 3:  // NFFT4GP_TRANSFORM_IDENTITY
      *tvalp = val;
      if (!inverse) *dtvalp = 1.0;
      break;
   default:
      printf("Error: unknown transform type.\n");
      return -1;
   }
   return 0;
}

int Nfft4GPGpLoss(double* x, double* data, double* label, int n, int ldim, int d, func_kernel fkernel,
                  void* vfkernel_data, func_free kernel_data_free, func_symmatvec matvec, func_symmatvec dmatvec,
                  func_kernel precond_fkernel, void* precond_vfkernel_data, func_free precond_vfkernel_data_free,
                  precond_kernel_setup precond_setup, func_solve precond_solve, func_trace precond_trace,
                  func_logdet precond_logdet, func_dvp precond_dvp, func_free precond_reset, void* precond_data,
                  int atol, double tol, int wsize, int maxits, int nvecs, double* radamacher,
                  nfft4gp_transform_type transform,
                  int* mask, int print_level, double* dwork, double* loss, double* grad)
{
   RandScope rand_scope;  // libc rand() as the reference draws it (internal.h)
   (void)precond_vfkernel_data_free;
   (void)wsize;
   if (!need_device("Nfft4GPGpLoss")) return -1;
   double tvals[3], dtvals[3];
   for (int i = 0; i < 3; i++)
      if (Nfft4GPTransform(transform, x[i], 0, tvals + i, dtvals + i)) return -1;
   printf("Transform %e %e %e into %e %e %e with grad %e %e %e\n", x[0], x[1], x[2], tvals[0], tvals[1], tvals[2],
          dtvals[0], dtvals[1], dtvals[2]);
   nfft4gp_kernel* kd = (nfft4gp_kernel*)vfkernel_data;
   nfft4gp_kernel* pkd = (nfft4gp_kernel*)precond_vfkernel_data;
   kd->_params[0] = tvals[0];
   kd->_params[1] = tvals[1];
   kd->_noise_level = tvals[2];
   if (pkd) {
      pkd->_params[0] = tvals[0];
      pkd->_params[1] = tvals[1];
      pkd->_noise_level = tvals[2];
   }
   double* kernel_mat = nullptr;
   double* dkernel_mat = nullptr;
   if (dwork) {
      kernel_mat = dwork;
      dkernel_mat = dwork + (size_t)n * n;
   }
   if (fkernel(vfkernel_data, data, n, ldim, d, nullptr, 0, nullptr, 0, &kernel_mat, &dkernel_mat)) return -1;
   if (precond_setup)
      precond_setup(data, n, ldim, d, precond_fkernel, precond_vfkernel_data, 1, precond_data);
   else
      precond_data = nullptr;

   Callbacks cb, dcb;
   if (!make_callbacks(cb, n, matvec, kernel_mat, precond_solve, precond_data) ||
       !make_callbacks(dcb, n, dmatvec, dkernel_mat, nullptr, nullptr))
      return -1;
   dcb.out_mult = 3;
   if (cb.comm != dcb.comm || cb.n_global != dcb.n_global) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPGpLoss: matvec and dmatvec must be split the same way\n");
      return -1;
   }
   const int nall = (int)cb.n_global;  // n of the whole problem (a row shard holds n of its rows)
   hipStream_t s = current_stream();
   Ctx c{s, (size_t)n, cb.comm};
   DevBuf<double> iKY, dKiKY;
   Vec vl;
   VecClose vl_close{vl};
   SyncOnExit sync{s};
   if (iKY.alloc((size_t)n) || dKiKY.alloc(3 * (size_t)n) || vl.open(label, n, true)) return -1;
   NFFT4GP_HIP_CHECK(hipMemsetAsync(iKY, 0, sizeof(double) * n, s));
   const int solve_kdim = std::min(nall, maxits * 2), solve_maxits = std::min(nall, maxits * 2);
   double rel_res, *rel_res_v = nullptr;
   int niter = 0;
   if (fgmres_dev(cb, iKY, vl.d, solve_kdim, solve_maxits, atol, tol, &rel_res, &rel_res_v, &niter, print_level))
      return -1;
   if (rel_res > 1e10) {
      printf("Warning: FGMRES unstable, rel_res = %f\n", rel_res);
      printf("Current parameters (after transform): f = %f, l = %f, mu = %f\n", tvals[0], tvals[1], tvals[2]);
   }
   free(rel_res_v);
   const double L1 = c.dot(vl.d, iKY) / (double)nall;
   if (dcb.apply(1.0, iKY, 0.0, dKiKY)) return -1;
   double L1_grad[3];
   for (int i = 0; i < 3; i++) L1_grad[i] = c.dot(dKiKY + (size_t)i * n, iKY) / (double)nall * dtvals[i];
   double L2 = 0.0, *L2_grad = nullptr;
   const int qits = std::min(nall, maxits);
   const int err = lanczos_logdet_dev(cb, dcb, precond_trace, precond_logdet, precond_dvp, qits, nvecs, radamacher,
                                      print_level, &L2, &L2_grad);
   if (err != 0) {
      printf("Error in Nfft4GPLanczosQuadratureLogdet\n");
      return err;
   }
   if (dist_final_check(cb)) {
      free(L2_grad);
      return -1;
   }
   loss[0] = 0.5 * (L1 + L2 + log(2.0 * 3.1415926535897932384626));
   for (int i = 0; i < 3; i++) {
      const double g = L2_grad ? 0.5 * (-L1_grad[i] + L2_grad[i] * dtvals[i]) : 0.0;
      grad[i] = (mask && !mask[i]) ? 0.0 : g;
   }
   free(L2_grad);
   if (!dwork && kernel_data_free) {
      kernel_data_free(kernel_mat);
      kernel_data_free(dkernel_mat);
   }
   if (precond_data && precond_reset) precond_reset(precond_data);
   return 0;
}

int Nfft4GPAdditiveNFFTGpPredict(double* x, double* data, double* label, int n, int ldim, int d,
                                 double* data_predict, int n_predict, int ldim_predict, double* data_all,
                                 func_kernel fkernel, void* vfkernel_data, void* vfkernel_data_l,
                                 func_free kernel_data_free, func_symmatvec matvec, func_kernel precond_fkernel,
                                 void* precond_vfkernel_data, func_free precond_kernel_data_free,
                                 precond_kernel_setup precond_setup, func_solve precond_solve, void* precond_data,
                                 int atol, double tol, int maxits, nfft4gp_transform_type transform,
                                 int print_level, double* dwork, double** label_predictp, double** std_predictp)
{
   (void)data_predict, (void)ldim_predict, (void)kernel_data_free, (void)precond_kernel_data_free, (void)dwork;
   if (!need_device("Nfft4GPAdditiveNFFTGpPredict")) return -1;
   double tvals[3], dtvals[3];
   for (int i = 0; i < 3; i++)
      if (Nfft4GPTransform(transform, x[i], 0, tvals + i, dtvals + i)) return -1;
   nfft4gp_kernel* kd = (nfft4gp_kernel*)vfkernel_data;
   nfft4gp_kernel* kl = (nfft4gp_kernel*)vfkernel_data_l;
   for (nfft4gp_kernel* k : {kd, kl}) {
      k->_params[0] = tvals[0];
      k->_params[1] = tvals[1];
      k->_noise_level = tvals[2];
   }
   double *K11 = nullptr, *dK11 = nullptr, *K = nullptr, *dK = nullptr;
   const int na = n + n_predict;
   if (fkernel(vfkernel_data, data, n, ldim, d, nullptr, 0, nullptr, 0, &K11, &dK11) ||
       fkernel(vfkernel_data_l, data_all, na, na, d, nullptr, 0, nullptr, 0, &K, &dK))
      return -1;
   if (precond_setup)
      precond_setup(data, n, ldim, d, precond_fkernel, precond_vfkernel_data, 1, precond_data);
   else
      precond_data = nullptr;
   Callbacks cb11, cba;
   if (!make_callbacks(cb11, n, matvec, K11, precond_solve, precond_data) ||
       !make_callbacks(cba, na, matvec, K, nullptr, nullptr))
      return -1;
   if (cb11.n_global != cb11.n || cb11.comm) {
      fprintf(stderr, "nfft4gp_amd: Nfft4GPAdditiveNFFTGpPredict takes a one-GPU operator\n");
      return -1;
   }
   hipStream_t s = current_stream();
   Ctx c{s, (size_t)n};
   DevBuf<double> iKY, helper;
   Vec vl;
   VecClose vl_close{vl};
   SyncOnExit sync{s};
   if (iKY.alloc((size_t)na) || helper.alloc((size_t)na) || vl.open(label, n, true)) return -1;
   NFFT4GP_HIP_CHECK(hipMemsetAsync(iKY, 0, sizeof(double) * na, s));
   double rel_res, *rel_res_v = nullptr;
   int niter = 0;
   if (fgmres_dev(cb11, iKY, vl.d, maxits, maxits, atol, tol, &rel_res, &rel_res_v, &niter, print_level)) return -1;
   free(rel_res_v);
   // label_predict = (K_all [iKY; 0])[n:]  (nfft_interface.c:973-979)
   if (cba.apply(1.0, iKY, 0.0, helper)) return -1;
   double* lp = *label_predictp ? *label_predictp : (double*)malloc(sizeof(double) * std::max(1, n_predict));
   const bool lp_dev = is_device_ptr(lp);
   NFFT4GP_HIP_CHECK(hipMemcpyAsync(lp, helper + n, sizeof(double) * n_predict,
                                    lp_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
   NFFT4GP_HIP_CHECK(hipStreamSynchronize(s));
   if (!*label_predictp) *label_predictp = lp;
   if (std_predictp) {
      // diag of K22 - K21 K11^{-1} K12 (nfft_interface.c:993-1060), a batch of prediction points at a time:
      // the K12 columns and K22 diagonal entries of the batch by one operator application to its unit vectors
      // (two per pass on this library's operator), then its solves K11 x = K12(:, i) in lockstep
      // (fgmres_batch_dev: restart dimension and iteration limit n as the reference), then the dots
      double* sp = *std_predictp ? *std_predictp : (double*)malloc(sizeof(double) * std::max(1, n_predict));
      std::vector<double> hs(n_predict);
      // 32 points per batch up to n = 2^18 (0.077 against 0.108 s for 16 at n = 20 000, 0.366 against 0.417 s at
      // n = 200 000: profiles/r05_predict_std_batch.txt), 16 above (each basis column holds batch x n doubles)
      int bm = n <= (1 << 18) ? 32 : 16;
      if (const char* e = getenv("NFFT4GP_AMD_PREDICT_BATCH")) bm = std::max(1, std::min(256, atoi(e)));
      bm = std::max(1, std::min(bm, n_predict));
      DevBuf<double> E, Y, Xs, dsc;
      BatchCtx dots(s, (size_t)n);  // the dots' partials, tickets and system list (gpart, gtick, dall)
      std::vector<int> ids(bm);
      for (int k = 0; k < bm; k++) ids[k] = k;
      if (E.alloc((size_t)na * bm) || Y.alloc((size_t)na * bm) || Xs.alloc((size_t)n * bm) ||
          dsc.alloc(2 * (size_t)bm) || dots.init(bm) || dots.set_active(ids)) {
         if (!*std_predictp) free(sp);
         return -1;
      }
      const bool multi = cba.mv_dev && cba.matvec == (func_symmatvec)&Nfft4GPAdditiveNFFTMatSymv;
      int rc = 0;
      for (int i0 = 0; i0 < n_predict && !rc; i0 += bm) {
         const int mb = std::min(bm, n_predict - i0);
         NFFT4GP_HIP_CHECK(hipMemsetAsync(E, 0, sizeof(double) * (size_t)na * mb, s));
         hipLaunchKernelGGL(k_set_units, dim3((mb + 255) / 256), dim3(256), 0, s, E, (size_t)na, (size_t)(n + i0), mb);
         std::vector<const double*> xs(mb);
         std::vector<double*> ys(mb);
         for (int k = 0; k < mb; k++) {
            xs[k] = E + (size_t)k * na;
            ys[k] = Y + (size_t)k * na;
         }
         if (multi) {
            rc = additive_matvec_multi(cba.mat, mb, 1.0, xs.data(), 0.0, ys.data());
         } else {
            for (int k = 0; k < mb && !rc; k++) rc = cba.apply(1.0, const_cast<double*>(xs[k]), 0.0, ys[k]);
         }
         if (rc) break;
         hipLaunchKernelGGL(k_pick_diag, dim3((mb + 255) / 256), dim3(256), 0, s, dsc, (const double*)Y, (size_t)na,
                            (size_t)(n + i0), mb);
         BatchOut bo;
         if ((rc = fgmres_batch_dev(cb11, mb, Xs, (size_t)n, Y, (size_t)na, n, n, atol, tol, print_level, bo))) break;
         // (K12(:, i), x_i) per point: k_gs_step's dot, batched
         if ((rc = dots.dot(Y, (size_t)na, Xs, (size_t)n, dsc + bm, mb))) break;
         std::vector<double> h2(2 * (size_t)bm);
         if ((rc = c.read(dsc, 2 * bm, h2.data()))) break;
         for (int k = 0; k < mb; k++) hs[i0 + k] = std::sqrt(std::fabs(h2[k] - h2[bm + k]));
      }
      if (rc) {
         if (!*std_predictp) free(sp);
         return -1;
      }
      if (is_device_ptr(sp))
         NFFT4GP_HIP_CHECK(hipMemcpy(sp, hs.data(), sizeof(double) * n_predict, hipMemcpyHostToDevice));
      else
         memcpy(sp, hs.data(), sizeof(double) * n_predict);
      if (!*std_predictp) *std_predictp = sp;
   }
   return 0;
}

}  // extern "C"
