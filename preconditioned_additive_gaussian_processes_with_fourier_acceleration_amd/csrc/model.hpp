// model.hpp -- the fitted model's state and the few functions its four files call across each other: model.hip (the
// table: lifetime, predict, effects), model_variance.hip (S and the predictive std), model_paths.hip (the sampler),
// model_centring.hip (the reference sample's means, the intercept).
#pragma once
#include <vector>

#include "internal.h"

namespace nfft4gp_amd {

struct Model {
   int nw = 0, d = 0, kernel = 0;
   double f = 1.0, l = 1.0, mu = 0.0;
   std::vector<double> centre, scale;  // host copies
   std::vector<int> feature;
   double* d_H = nullptr;       // [nw][64][kNC]
   double* d_centre = nullptr;  // [nw]
   double* d_scale = nullptr;   // [nw]
   int* d_feature = nullptr;    // [nw]
   BlockCounts counts;          // per-workgroup counts of outside points
   double* d_S = nullptr;  // the variance matrix, mv_order(nw)^2, symmetric, windows kMvPad slots apart; or none
   int R = 0;              // 33 nw once a variance is held, else 0
   double fit_ms[3] = {0.0, 0.0, 0.0};  // the last fit's wall clock: features, Grams and their sum, system + LU
   // the sampler (model_paths.hip): S+ = F F^T and the drawn paths' weights B = F xi
   double* d_Ft = nullptr;  // F^T, R x R_p column-major: column slot(j) is F's row j, the padded slots' columns zero
   double* d_Bt = nullptr;  // B^T, nsp x R_p column-major, nsp = ns rounded up to the sample tile; rows >= ns zero
   int ns = 0, nsp = 0;
   double defect = 0.0, lam_min = 0.0, lam_max = 0.0;  // sum |lambda < 0| / sum |lambda| and S's extreme eigenvalues
   double sampler_ms = 0.0;                            // the eigendecomposition's wall clock
   // the centring on a reference sample (model_centring.hip): it belongs to the table and the sample, not
   // to S, so a new variance keeps it
   double* d_fmean = nullptr;   // m = Z^T 1 / n_ref in S's slot layout: mv_order(nw), the padded slots zero; or none
   double* d_emean = nullptr;   // [nw] the effects' means over the sample
   std::vector<double> emean, esd;  // host copies: the effects' means and their standard deviations over the sample
   int n_ref = 0;                   // the sample's rows; 0: no centring held
};

inline WindowMap window_map(const Model* M) { return WindowMap{M->nw, M->d, M->d_centre, M->d_scale, M->d_feature}; }

template <class T>
int to_device(T** dptr, const T* h, size_t count)
{
   NFFT4GP_HIP_CHECK(hipMalloc((void**)dptr, sizeof(T) * std::max<size_t>(1, count)));
   NFFT4GP_HIP_CHECK(hipMemcpy(*dptr, h, sizeof(T) * count, hipMemcpyHostToDevice));
   return 0;
}

// S has changed or goes: the factor of the old one and the paths drawn from it go with it (model.hip)
void model_drop_sampler(Model* M);
// the posterior mean at the rows of Xnew (host or device); *n_outside (may be NULL): the rows outside the domain
int model_predict(Model* M, const double* Xnew, int n_new, long long ldim, double* mean, long long* n_outside);
// the windows [w0, w0 + wn) one by one: their effects and, with effect_std, the effects' standard deviations; centred:
// both about the reference sample's means (the model holds a centring then)
int model_predict_effects(Model* M, const double* Xnew, int n_new, long long ldim, int w0, int wn, double* effects,
                          double* effect_std, long long ldo, long long* n_outside, bool centred = false);
// the centring goes (model_centring.hip)
void model_drop_centring(Model* M);

}  // namespace nfft4gp_amd
