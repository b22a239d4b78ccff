// nfn_meanfield.hip — the mean-field posterior of every DenseVariational weight at once
// (MeanFieldLayer, estimators/DistributionLayers.py:17-71; BayesianNNEstimator.py:78-107):
// the draw w = loc + s * eps, KL(q || p) against the prior Normal(prior_loc, prior_scale),
// and the gradients of both, over ONE flat vector of all N weights of the network.
//
//   x = log(e - 1) + 0.05 rho,  s = 1e-3 + softplus(x)
//   exact KL term    log(sp / s) + (s^2 + (m - p)^2) / (2 sp^2) - 1/2
//   sampled KL term  -log s - eps^2 / 2 + log sp + (w - p)^2 / (2 sp^2)     (log q(w) - log p(w))
//   map mode (no rho, no eps): q = Normal(loc, 1) converted by its mean, w = m
//
// s and log s are fp32 (the OCML softplus of the base distribution, one form for both math
// modes); every KL term is assembled and summed in fp64 from those fp32 values: near s ~ sp,
// m ~ p a term is a difference of O(1) parts.  The sum leaves through write_partial.  The
// backward assembles in fp64 too, and for the sampled KL takes s itself in fp64 (mf_backward).
//
// Both kernels are grid-stride loops over groups of four elements.  The groups start at the
// first element at which `loc` is 16-byte aligned; every other array moves 16 bytes per lane
// where its own address at that element is aligned too, and four dwords where it is not (the
// arrays are separate allocations and views: there is no common phase).  The at most three
// elements before the first group and after the last are handled one by one.
#include "nfn_launch.h"

namespace nfn {
namespace {

// bit of MeanFieldArgs::vec per array
enum : uint32_t {
  kVecLoc = 1u, kVecRho = 2u, kVecEps = 4u, kVecPrior = 8u, kVecGw = 16u,
  kVecOutW = 32u, kVecGradLoc = 64u, kVecGradRho = 128u, kVecGradPrior = 256u,
};

__device__ __forceinline__ f32x4 load4(const float* p, bool vec) {
  f32x4 v;
  if (vec) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
    v.x = p[0];
    v.y = p[1];
    v.z = p[2];
    v.w = p[3];
  }
  return v;
}

__device__ __forceinline__ void store4(float* p, bool vec, f32x4 v) {
  if (vec) {
    *reinterpret_cast<f32x4*>(p) = v;
  } else {
    p[0] = v.x;
    p[1] = v.y;
    p[2] = v.z;
    p[3] = v.w;
  }
}

// The posterior scale and the argument of its softplus.
__device__ __forceinline__ float mf_scale(float rho, float& x) {
  x = fmaf(0.05f, rho, kLogExpm1One);
  return 1e-3f + softplus_tf<false>(x);
}

// The same scale in fp64 (the softplus in its stable form; TF's thresholds cut it below fp32's
// resolution only): for the backward of the sampled KL.
__device__ __forceinline__ double mf_scale64(float rho) {
  const double x = fma(0.05, (double)rho, 0.54132485461291810);
  return 1e-3 + (fmax(x, 0.0) + log1p(exp(-fabs(x))));
}

// One element of the forward: the draw and its KL term.
template <bool MAP>
__device__ __forceinline__ float mf_forward(float m, float rho, float eps, float p, const MeanFieldArgs& a,
                                            double& term) {
  const double dm = (double)m - (double)p;
  if constexpr (MAP) {
    term = a.kl_exact ? fma(fma(dm, dm, 1.0), a.inv_2var, a.log_ps - 0.5) : fma(dm * dm, a.inv_2var, a.log_ps);
    return m;
  } else {
    float x;
    const float s = mf_scale(rho, x);
    const double sd = (double)s, ls = (double)logf(s);
    if (a.kl_exact) {
      term = fma(fma(sd, sd, dm * dm), a.inv_2var, (a.log_ps - ls) - 0.5);
    } else {
      const double e = (double)eps, dw = fma(sd, e, dm);  // w - p at the same draw
      term = fma(dw * dw, a.inv_2var, (a.log_ps - ls) - 0.5 * e * e);
    }
    return fmaf(s, eps, m);
  }
}

// One element of the backward: (grad_loc, grad_rho, grad_prior_loc) from the upstream
// gradients gw (of the draw) and gk (of the KL sum).
template <bool MAP>
__device__ __forceinline__ void mf_backward(float m, float rho, float eps, float p, float gw, double gk,
                                            const MeanFieldArgs& a, float& g_loc, float& g_rho, float& g_prior) {
  const double dm = (double)m - (double)p;
  const double inv_var = 2.0 * a.inv_2var;
  if constexpr (MAP) {
    const double A = gk * dm * inv_var;
    g_loc = (float)((double)gw + A);
    g_rho = 0.0f;
    g_prior = (float)(-A);
  } else {
    float x;
    const float s = mf_scale(rho, x);
    const float dsig = 0.05f / (1.0f + expf(-x));  // ds / drho = 0.05 sigmoid(x)
    const double e = (double)eps;
    double A, Bs;
    if (a.kl_exact) {
      const double sd = (double)s;
      A = dm * inv_var;
      Bs = fma(sd, inv_var, -1.0 / sd);
    } else {
      // w - p = (m - p) + s eps cancels where the draw lands on the prior mean, and the
      // rounding of an fp32 s (1e-6 at s = 20) times eps / sp^2 is then the whole gradient:
      // measured on 2.1e6 elements at sp = 0.1, 29 left 1e-5 max(1, |ref|), the worst at 1.9
      // times it.  The sampled form takes s in fp64.
      const double sd = mf_scale64(rho);
      A = fma(sd, e, dm) * inv_var;
      Bs = fma(e, A, -1.0 / sd);
    }
    A *= gk;
    g_loc = (float)((double)gw + A);
    g_rho = (float)(fma((double)gw, e, gk * Bs) * (double)dsig);
    g_prior = (float)(-A);
  }
}

// The element of the `k`-th scalar slot: the head's elements first, then the tail's.
__device__ __forceinline__ int64_t mf_scalar_index(const MeanFieldArgs& a, int k) {
  return k < a.head ? (int64_t)k : (int64_t)a.head + 4 * a.nvec + (k - a.head);
}

template <bool MAP>
__global__ void __launch_bounds__(kMaxBlock) mean_field_draw_kl_kernel(MeanFieldArgs a) {
  __shared__ double red[2 * kMaxBlock / 64];
  double acc = 0.0;
  int nfc = 0;
  const float* loc = a.loc + a.head;
  [[maybe_unused]] const float* rho = MAP ? nullptr : a.rho + a.head;
  [[maybe_unused]] const float* eps = MAP ? nullptr : a.eps + a.head;
  const float* prior = a.prior_loc ? a.prior_loc + a.head : nullptr;
  float* out_w = a.out_w ? a.out_w + a.head : nullptr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.nvec; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 4 * g;
    const f32x4 m = load4(loc + i, a.vec & kVecLoc);
    f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f}, e = r, p = r, w;
    if constexpr (!MAP) {
      r = load4(rho + i, a.vec & kVecRho);
      e = load4(eps + i, a.vec & kVecEps);
    }
    if (prior) p = load4(prior + i, a.vec & kVecPrior);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double term;
      w[j] = mf_forward<MAP>(m[j], r[j], e[j], p[j], a, term);
      acc += term;
      nfc += __builtin_isfinite(term) ? 0 : 1;
    }
    if (out_w) store4(out_w + i, a.vec & kVecOutW, w);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < a.head + a.tail) {
    const int64_t i = mf_scalar_index(a, (int)threadIdx.x);
    double term;
    const float w = mf_forward<MAP>(a.loc[i], MAP ? 0.0f : a.rho[i], MAP ? 0.0f : a.eps[i],
                                    a.prior_loc ? a.prior_loc[i] : 0.0f, a, term);
    acc += term;
    nfc += __builtin_isfinite(term) ? 0 : 1;
    if (a.out_w) a.out_w[i] = w;
  }
  if (a.partials) write_partial(a.partials, acc, nfc, red, a.out_sum, a.epoch);
}

template <bool MAP>
__global__ void __launch_bounds__(kMaxBlock) mean_field_draw_kl_grad_kernel(MeanFieldArgs a) {
  const double gk = a.g_kl ? (double)a.g_kl[0] : 0.0;
  const float* loc = a.loc + a.head;
  [[maybe_unused]] const float* rho = MAP ? nullptr : a.rho + a.head;
  [[maybe_unused]] const float* eps = MAP ? nullptr : a.eps + a.head;
  const float* prior = a.prior_loc ? a.prior_loc + a.head : nullptr;
  const float* g_w = a.g_w ? a.g_w + a.head : nullptr;
  float* grad_loc = a.grad_loc ? a.grad_loc + a.head : nullptr;
  float* grad_rho = (!MAP && a.grad_rho) ? a.grad_rho + a.head : nullptr;
  float* grad_prior = a.grad_prior_loc ? a.grad_prior_loc + a.head : nullptr;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < a.nvec; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = 4 * g;
    const f32x4 m = load4(loc + i, a.vec & kVecLoc);
    f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f}, e = r, p = r, gw = r, gl, gr, gp;
    if constexpr (!MAP) {
      r = load4(rho + i, a.vec & kVecRho);
      e = load4(eps + i, a.vec & kVecEps);
    }
    if (prior) p = load4(prior + i, a.vec & kVecPrior);
    if (g_w) gw = load4(g_w + i, a.vec & kVecGw);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x, y, z;
      mf_backward<MAP>(m[j], r[j], e[j], p[j], gw[j], gk, a, x, y, z);
      gl[j] = x;
      gr[j] = y;
      gp[j] = z;
    }
    if (grad_loc) store4(grad_loc + i, a.vec & kVecGradLoc, gl);
    if (grad_rho) store4(grad_rho + i, a.vec & kVecGradRho, gr);
    if (grad_prior) store4(grad_prior + i, a.vec & kVecGradPrior, gp);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < a.head + a.tail) {
    const int64_t i = mf_scalar_index(a, (int)threadIdx.x);
    float gl, gr, gp;
    mf_backward<MAP>(a.loc[i], MAP ? 0.0f : a.rho[i], MAP ? 0.0f : a.eps[i], a.prior_loc ? a.prior_loc[i] : 0.0f,
                     a.g_w ? a.g_w[i] : 0.0f, gk, a, gl, gr, gp);
    if (a.grad_loc) a.grad_loc[i] = gl;
    if (!MAP && a.grad_rho) a.grad_rho[i] = gr;
    if (a.grad_prior_loc) a.grad_prior_loc[i] = gp;
  }
}

// `p + head` is 16-byte aligned (a NULL array takes no path at all).
uint32_t vec_bit(const void* p, int head, uint32_t bit) {
  return p && ((reinterpret_cast<uintptr_t>(p) + 4u * (uintptr_t)head) & 15u) == 0 ? bit : 0u;
}

}  // namespace

int64_t launch_mean_field(bool grad, const MeanFieldArgs& a0, hipStream_t s) {
  MeanFieldArgs a = a0;
  // elements before the first 16-byte boundary of loc (float arrays are 4-byte aligned)
  const int phase = (int)((reinterpret_cast<uintptr_t>(a.loc) >> 2) & 3u);
  a.head = (int32_t)std::min<int64_t>((4 - phase) & 3, a.N);
  a.nvec = (a.N - a.head) / 4;
  a.tail = (int32_t)(a.N - a.head - 4 * a.nvec);
  a.vec = vec_bit(a.loc, a.head, kVecLoc) | vec_bit(a.rho, a.head, kVecRho) | vec_bit(a.eps, a.head, kVecEps) |
          vec_bit(a.prior_loc, a.head, kVecPrior) | vec_bit(a.g_w, a.head, kVecGw) |
          vec_bit(a.out_w, a.head, kVecOutW) | vec_bit(a.grad_loc, a.head, kVecGradLoc) |
          vec_bit(a.grad_rho, a.head, kVecGradRho) | vec_bit(a.grad_prior_loc, a.head, kVecGradPrior);
  const bool map = a.rho == nullptr;
  const int64_t units = std::max<int64_t>(1, (a.nvec + kMaxBlock - 1) / kMaxBlock);
  int64_t grid;
  if (grad) {
    auto kfn = map ? mean_field_draw_kl_grad_kernel<true> : mean_field_draw_kl_grad_kernel<false>;
    grid = std::max<int64_t>(1, std::min(persistent_grid(kfn, kMaxBlock, 0, units), a.grid_cap));
    nfn_launch(kfn, dim3((unsigned)grid), dim3(kMaxBlock), 0u, s, a);
  } else {
    auto kfn = map ? mean_field_draw_kl_kernel<true> : mean_field_draw_kl_kernel<false>;
    grid = std::max<int64_t>(1, std::min(persistent_grid(kfn, kMaxBlock, 0, units), a.grid_cap));
    nfn_launch(kfn, dim3((unsigned)grid), dim3(kMaxBlock), 0u, s, a);
  }
  return grid;
}

}  // namespace nfn
