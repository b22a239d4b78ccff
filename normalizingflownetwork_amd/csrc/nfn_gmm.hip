// nfn_gmm.hip — the mixture density network's density layer (GaussianMixtureLayer,
// estimators/DistributionLayers.py:174-212): log_prob of a mixture of K diagonal Gaussians
// whose locations, scales and weights all come out of the parameter row, forward and
// backward.  Compiled twice: -DNFN_FAST=1 and -DNFN_FAST=0.
//
//   row t (P = 2 K d + K):  [loc_0 (d) | raw_0 (d) | ... | loc_{K-1} | raw_{K-1} | logits (K)]
//   sigma_kj = softplus(0.05 raw_kj + log(expm1(1))),  z_kj = (y_j - loc_kj) / sigma_kj
//   c_k      = -0.5 sum_j z_kj^2 - sum_j log sigma_kj - 0.5 d log(2 pi)
//   logp     = logsumexp_k(l_k + c_k) - logsumexp_k(l_k)
//
// Each LANE owns a whole row: a wave owns tiles of R rows (R = 64, 32 or 16 by row width),
// streams a tile's contiguous span into LDS with coalesced loads at the odd row stride P | 1
// (lane r then walks row r free of bank conflicts), and every lane evaluates its row's K
// components serially.  No cross-lane reduction and no workgroup barrier in the tile loop.
// The log-sum-exp is shifted: m_l = max_k l_k first, then one pass with u_k = l_k - m_l,
// sum exp(u_k) and an online log-sum-exp of a_k = u_k + c_k, so no term of magnitude |l| is
// ever subtracted from another; what has the magnitude of c_k is carried in fp64 (gmm_z).
// The backward runs the same pass for the two normalisers, then overwrites each parameter in
// its LDS row with its gradient and streams the tile out.
#include "nfn_launch.h"

#ifndef NFN_FAST
#error "compile with -DNFN_FAST=0 or -DNFN_FAST=1"
#endif

namespace nfn {
namespace {

constexpr bool kFast = NFN_FAST != 0;
constexpr int kGmmLdsBudget = 64 * 1024;  // bytes of tiles per workgroup that set the waves per workgroup

// A wave's walk over a tile's (rows x W) pieces, piece i = lane + 64 n at (row i / W, column
// i % W): the lane's first piece and the step of 64 pieces, fixed for the whole launch.
struct WaveWalk {
  int r0, c0, sr, sc, W;
};
__device__ __forceinline__ WaveWalk make_walk(int W, int lane) {
  WaveWalk w;
  w.W = W;
  w.r0 = lane / W;
  w.c0 = lane - w.r0 * W;
  w.sr = 64 / W;
  w.sc = 64 - w.sr * W;
  return w;
}
__device__ __forceinline__ void walk_step(const WaveWalk& w, int& r, int& c) {
  r += w.sr;
  c += w.sc;
  if (c >= w.W) {
    c -= w.W;
    r += 1;
  }
}

// Stream `nr` rows (global row stride rs floats; 0 = one row for all) into the wave's LDS
// rows of stride S.  VEC: 16-byte pieces (the caller checked width, stride and alignment).
// Four loads per lane are in flight before the first LDS write.
template <bool VEC>
__device__ __forceinline__ void wave_stage(float* tl, const float* __restrict__ src, int64_t rs, int nr, int S,
                                           const WaveWalk& w, int lane) {
  constexpr int U = 4;
  const int n = nr * w.W;
  int r = w.r0, c = w.c0;
  for (int i = lane; i < n; i += 64 * U) {
    int off[U];
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i + 64 * u < n) {
        if constexpr (VEC) {
          off[u] = r * S + 4 * c;
          v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + (int64_t)r * rs + 4 * c));
        } else {
          off[u] = r * S + c;
          v[u].x = __builtin_nontemporal_load(src + (int64_t)r * rs + c);
        }
      }
      walk_step(w, r, c);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i + 64 * u < n) {
        tl[off[u]] = v[u].x;
        if constexpr (VEC) {
          tl[off[u] + 1] = v[u].y;
          tl[off[u] + 2] = v[u].z;
          tl[off[u] + 3] = v[u].w;
        }
      }
    }
  }
}

// The way back: the wave's LDS rows to `nr` global rows, the same walk.
template <bool VEC>
__device__ __forceinline__ void wave_unstage(const float* tl, float* __restrict__ dst, int64_t rs, int nr, int S,
                                             const WaveWalk& w, int lane) {
  const int n = nr * w.W;
  int r = w.r0, c = w.c0;
  for (int i = lane; i < n; i += 64) {
    if constexpr (VEC) {
      const float* p = tl + r * S + 4 * c;
      f32x4 v;
      v.x = p[0];
      v.y = p[1];
      v.z = p[2];
      v.w = p[3];
      __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(dst + (int64_t)r * rs + 4 * c));
    } else {
      __builtin_nontemporal_store(tl[r * S + c], dst + (int64_t)r * rs + c);
    }
    walk_step(w, r, c);
  }
}

// c_k moves by z^2 times the relative error of sigma and of z = (y - loc) / sigma, and the
// posterior weights are exponentials of differences of the c_k, which reach 1e4 and more
// (|y| or |loc| of 30).  Measured with everything in fp32 (hardware log / exp / rcp): stress
// gradients at 6.7 times the fp32 mirror's own deviation; with the OCML softplus and a
// correctly rounded quotient still 5.4 times on one case, the remaining roundings at the
// magnitude of c_k.  So:
//  * sigma is the OCML softplus in BOTH math modes (expf / log1pf: about half an ulp, and
//    RELATIVE accuracy as its argument falls — there is no floor under sigma; the fast
//    softplus rounds to 0 below about -16.6);
//  * everything of magnitude c_k is fp64: y - loc, the quotient (v_rcp_f32 and one Newton
//    step in fp64), the sum of squares, c_k, a_k = u_k + c_k and the running maximum M, so
//    a_k - M is rounded to fp32 once, as a small number.
// What is left is sigma's own fp32 rounding, which the mirror has too.  Fast math keeps the
// hardware transcendentals everywhere else (log sigma, the exponentials, the sigmoid).
__device__ __forceinline__ float gmm_sigma(float raw, float& x) {
  x = fmaf(0.05f, raw, kLogExpm1One);
  return softplus_tf<false>(x);
}

__device__ __forceinline__ double gmm_z(float y, float loc, float sg) {
  const double s = (double)sg;
  double r = (double)__builtin_amdgcn_rcpf(sg);
  r = fma(fma(-s, r, 1.0), r, r);
  return ((double)y - (double)loc) * r;
}

// log-density of component k (parameters at p: loc (d), raw (d)) at the lane's (normalised)
// y: c_k.  STASH (the backward's second pass) also overwrites the component's slots with the
// factors of its gradients, z / sigma over loc_j and (z^2 - 1) / sigma * 0.05 sigmoid(x) over
// raw_j.
template <bool FAST, bool STASH>
__device__ __forceinline__ double gmm_component(std::conditional_t<STASH, float*, const float*> p, const float* ys,
                                                int d) {
  double q = 0.0;
  float ls = 0.0f;
  for (int j = 0; j < d; ++j) {
    float x;
    const float sg = gmm_sigma(p[d + j], x);
    const double zd = gmm_z(ys[j], p[j], sg);
    q = fma(zd, zd, q);
    ls += f_log<FAST>(sg);
    if constexpr (STASH) {
      const float z = (float)zd;
      const float sig = f_div<FAST>(1.0f, 1.0f + f_exp<FAST>(-x));
      p[j] = f_div<FAST>(z, sg);
      p[d + j] = fmaf(z, z, -1.0f) * f_div<FAST>(0.05f * sig, sg);
    }
  }
  return fma(-0.5, q, -(double)(ls + (float)d * kHalfLog2Pi));
}

// u_k = l_k - m_l; a -inf logit stays -inf (never -inf - -inf).
__device__ __forceinline__ float gmm_shift(float l, float ml) { return l == -INFINITY ? -INFINITY : l - ml; }

// lse_push (nfn_device.h) with the running maximum in fp64: branch-free, one exp per term; a
// -inf term changes nothing, a NaN makes M NaN.
template <bool FAST>
__device__ __forceinline__ void gmm_push(double& M, float& acc, double av) {
  const float dlt = (float)(av - M);
  const float e = f_exp<FAST>(-fabsf(dlt));
  const bool up = dlt > 0.0f;  // false for NaN
  const float acc_new = up ? fmaf(acc, e, 1.0f) : acc + e;
  acc = (av == -INFINITY) ? acc : acc_new;
  M = (av != av) ? av : (up ? av : M);
}

// One row: m_l = max_k l_k, s0 = sum_k exp(u_k), and (M, acc) the online log-sum-exp of
// a_k = u_k + c_k (logsumexp_k a = M + log acc).  Returns logp without the y_std term.
template <bool FAST>
__device__ __forceinline__ float gmm_row(const float* row, const float* ys, int K, int d, float& ml, float& s0,
                                         double& M, float& acc) {
  const float* lg = row + 2 * K * d;
  ml = -INFINITY;
  for (int k = 0; k < K; ++k) ml = fmaxf(ml, lg[k]);  // drops a NaN: it comes back through u_k
  s0 = 0.0f;
  M = -(double)INFINITY;
  acc = 0.0f;
  for (int k = 0; k < K; ++k) {
    const double c = gmm_component<FAST, false>(row + 2 * k * d, ys, d);
    const float u = gmm_shift(lg[k], ml);
    s0 += f_exp<FAST>(u);
    gmm_push<FAST>(M, acc, (double)u + c);
  }
  return (float)(M + (double)f_log<FAST>(acc)) - f_log<FAST>(s0);
}

// Stage nr rows of t from src into the wave's LDS rows, in 16-byte pieces where the launcher
// found that the rows allow it.
__device__ __forceinline__ void gmm_stage_t(float* tl, const GmmArgs& a, const float* src, int nr, const WaveWalk& wt,
                                            int lane) {
  if (a.vec4)
    wave_stage<true>(tl, src, a.rs, nr, a.S, wt, lane);
  else
    wave_stage<false>(tl, src, a.rs, nr, a.S, wt, lane);
}

// the lane's staged y, normalised in place
template <bool FAST>
__device__ __forceinline__ void gmm_normalise_y(float* ys, const GmmArgs& a) {
  if (a.y_mean) {
    for (int j = 0; j < a.d; ++j) ys[j] = f_div_acc<FAST>(ys[j] - a.y_mean[j], a.y_std[j]);
  }
}

template <bool FAST, bool GRAD>
__global__ void __launch_bounds__(kMaxBlock) gaussian_mixture_kernel(GmmArgs a) {
  extern __shared__ float lds[];
  __shared__ double red[2 * kMaxBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int K = a.K, d = a.d, P = a.P, S = a.S, Sy = a.Sy, R = a.R;
  float* tl = lds + wid * (R * (S + Sy));  // this wave's rows of t, then its rows of y
  float* yl = tl + R * S;
  float* row = tl + lane * S;
  float* ys = yl + lane * Sy;
  const WaveWalk wt = make_walk(a.vec4 ? P >> 2 : P, lane);
  const WaveWalk wy = make_walk(d, lane);
  const float corr = log_std_sum<FAST>(a.y_mean, a.y_std, d);
  double acc_sum = 0.0;
  int nfc = 0;
  for (int64_t tile = (int64_t)blockIdx.x * nw + wid; tile < a.ntiles; tile += (int64_t)gridDim.x * nw) {
    const int64_t b0 = tile * R;
    const int nr = (int)min((int64_t)R, a.B - b0);
    const float* src = a.t + b0 * a.rs;
    gmm_stage_t(tl, a, src, nr, wt, lane);
    wave_stage<false>(yl, a.y + b0 * a.y_bstride, a.y_bstride, nr, Sy, wy, lane);
    [[maybe_unused]] float g = 0.0f;
    if constexpr (GRAD) {
      if (lane < nr) g = a.g_out ? a.g_out[b0 + lane] : 1.0f;
    }
    wave_lds_sync();
    if (lane < nr) {
      const int64_t b = b0 + lane;
      gmm_normalise_y<FAST>(ys, a);
      float ml, s0, acc;
      double M;
      const float lp = gmm_row<FAST>(row, ys, K, d, ml, s0, M, acc) - corr;
      if (a.out) a.out[b] = lp;
      if constexpr (!GRAD) {
        acc_sum += (double)lp;
        nfc += nonfinite1(lp);
      } else {
        // pass 2: every parameter is overwritten in place with its gradient
        const float r0 = f_div<FAST>(1.0f, s0), r1 = f_div<FAST>(1.0f, acc);
        float* lg = row + 2 * K * d;
        for (int k = 0; k < K; ++k) {
          float* p = row + 2 * k * d;
          const double c = gmm_component<FAST, true>(p, ys, d);  // leaves its factors in p
          const float u = gmm_shift(lg[k], ml);
          const double av = (double)u + c;
          // a removed component (and one whose weight underflows) gets exact zeros through
          // selects: its stashed factors may be inf
          const float post = av == -INFINITY ? 0.0f : f_exp<FAST>((float)(av - M)) * r1;
          lg[k] = g * (post - f_exp<FAST>(u) * r0);
          const float gp = g * post;
          const bool dead = post == 0.0f;
          for (int j = 0; j < 2 * d; ++j) p[j] = dead ? 0.0f : gp * p[j];
        }
        if (a.grad_y) {  // dL/dy_j = -sum_k dL/dloc_kj
          for (int j = 0; j < d; ++j) {
            float sy = 0.0f;
            for (int k = 0; k < K; ++k) sy += row[2 * k * d + j];
            a.grad_y[b * d + j] = a.y_mean ? f_div<FAST>(-sy, a.y_std[j]) : -sy;
          }
        }
      }
    }
    if constexpr (GRAD) {
      if (a.grad_t) {
        wave_lds_sync();
        float* dst = a.grad_t + b0 * a.gt_rs;
        if (a.gt_vec4)
          wave_unstage<true>(tl, dst, a.gt_rs, nr, S, wt, lane);
        else
          wave_unstage<false>(tl, dst, a.gt_rs, nr, S, make_walk(P, lane), lane);
      }
    }
    wave_lds_sync();  // the tile's LDS reads are done before the next tile is staged
  }
  if constexpr (!GRAD) {
    if (a.partials) write_partial(a.partials, acc_sum, nfc, red, a.out_sum, a.epoch);
  }
}

// The posterior score (BayesianNNEstimator.score, BayesianNNEstimator.py:65-76) of the same
// layer: logsumexp over a.nd draws of the row's log_prob, minus log S.  The layout of
// gaussian_mixture_kernel: a tile's y is staged and normalised once, then draw after draw
// the tile's rows are staged and every lane pushes its gmm_row into its own running (m, acc)
// (lse_push / lse_finish, nfn_device.h).  One float per sample leaves the kernel.
// The row's formula is gmm_row's and the staging is gmm_stage_t / gmm_normalise_y.  The opening
// lines (wave pointers, walks, corr) are written as in gaussian_mixture_kernel, not shared with
// it: built in one helper, this kernel ran the same loops 0.9 % slower on the small-batch score
// (K = 5, B = 2048, S = 50); as it stands its code is what it was before the helpers.
template <bool FAST>
__global__ void __launch_bounds__(kMaxBlock) gaussian_mixture_posterior_kernel(GmmArgs a) {
  extern __shared__ float lds[];
  __shared__ double red[2 * kMaxBlock / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int K = a.K, d = a.d, P = a.P, S = a.S, Sy = a.Sy, R = a.R;
  float* tl = lds + wid * (R * (S + Sy));  // this wave's rows of t, then its rows of y
  float* yl = tl + R * S;
  float* row = tl + lane * S;
  float* ys = yl + lane * Sy;
  const WaveWalk wt = make_walk(a.vec4 ? P >> 2 : P, lane);
  const WaveWalk wy = make_walk(d, lane);
  float corr = 0.0f;
  if (a.y_mean) {
    for (int j = 0; j < d; ++j) corr += f_log<FAST>(a.y_std[j]);
  }
  double acc_sum = 0.0;
  int nfc = 0;
  for (int64_t tile = (int64_t)blockIdx.x * nw + wid; tile < a.ntiles; tile += (int64_t)gridDim.x * nw) {
    const int64_t b0 = tile * R;
    const int nr = (int)min((int64_t)R, a.B - b0);
    wave_stage<false>(yl, a.y + b0 * a.y_bstride, a.y_bstride, nr, Sy, wy, lane);
    wave_lds_sync();
    if (lane < nr) gmm_normalise_y<FAST>(ys, a);
    float m = -INFINITY, lacc = 0.0f;
    for (int s = 0; s < a.nd; ++s) {
      const float* src = a.t + (int64_t)s * a.ds + b0 * a.rs;
      gmm_stage_t(tl, a, src, nr, wt, lane);
      wave_lds_sync();
      if (lane < nr) {
        float ml, s0, acc;
        double M;
        float lp = gmm_row<FAST>(row, ys, K, d, ml, s0, M, acc) - corr;
        // every logit -inf (s0 is exactly 0 then, and only then): the draw has no component
        // left, its term is -inf and drops out (the single-draw entry gives NaN, -inf - -inf)
        lp = s0 == 0.0f ? -INFINITY : lp;
        lse_push<FAST>(m, lacc, lp);
      }
      wave_lds_sync();  // this draw's LDS reads are done before the next draw (or tile) is staged
    }
    if (lane < nr) {
      const float res = lse_finish<FAST>(m, lacc, a.nd);
      if (a.out) a.out[b0 + lane] = res;
      acc_sum += (double)res;
      nfc += nonfinite1(res);
    }
  }
  if (a.partials) write_partial(a.partials, acc_sum, nfc, red, a.out_sum, a.epoch);
}

// Tile geometry of a launch: the LDS strides, the rows per wave tile and the tile count into
// `a`; returns the waves per workgroup (0: the shape has no launch) and the LDS bytes.
int gmm_geometry(GmmArgs& a, size_t& lds) {
  a.S = a.P | 1;
  a.Sy = a.d | 1;
  // rows per wave tile: 64 while 64 rows of P | 1 floats fit 64 KB, then 32, then 16 (P <= 1023)
  a.R = a.S <= 255 ? 64 : (a.S <= 511 ? 32 : 16);
  const size_t wave_bytes = sizeof(float) * (size_t)a.R * (size_t)(a.S + a.Sy);
  const int waves = (int)std::max<size_t>(1, std::min<size_t>(kMaxBlock / 64, kGmmLdsBudget / wave_bytes));
  lds = wave_bytes * waves;
  if (lds > (size_t)kLdsMaxBytes) return 0;
  // the 16-byte path only where the rows allow it (P is odd whenever K is: dwords are the rule)
  const bool v4 = (a.P & 3) == 0;
  a.vec4 = v4 && (a.rs & 3) == 0 && (a.ds & 3) == 0 && (reinterpret_cast<uintptr_t>(a.t) & 15) == 0;
  a.ntiles = (a.B + a.R - 1) / a.R;
  return waves;
}

template <typename KFN>
int64_t launch_gmm_kernel(KFN kfn, const GmmArgs& a, int waves, size_t lds, hipStream_t s) {
  int64_t grid = persistent_grid(kfn, 64 * waves, lds, (a.ntiles + waves - 1) / waves);
  grid = std::max<int64_t>(1, std::min(grid, a.grid_cap));
  nfn_launch(kfn, dim3((unsigned)grid), dim3((unsigned)(64 * waves)), (uint32_t)lds, s, a);
  return grid;
}

template <bool GRAD>
int64_t launch_gmm(const GmmArgs& a0, hipStream_t s) {
  GmmArgs a = a0;
  size_t lds;
  const int waves = gmm_geometry(a, lds);
  if (waves == 0) return 0;
  a.gt_vec4 = a.vec4 && a.grad_t && (a.gt_rs & 3) == 0 && (reinterpret_cast<uintptr_t>(a.grad_t) & 15) == 0;
  return launch_gmm_kernel(gaussian_mixture_kernel<kFast, GRAD>, a, waves, lds, s);
}

int64_t launch_gmm_posterior(const GmmArgs& a0, hipStream_t s) {
  GmmArgs a = a0;
  size_t lds;
  const int waves = gmm_geometry(a, lds);
  if (waves == 0) return 0;
  return launch_gmm_kernel(gaussian_mixture_posterior_kernel<kFast>, a, waves, lds, s);
}

}  // namespace

#if NFN_FAST
int64_t launch_gmm_fast(bool grad, const GmmArgs& a, hipStream_t s) {
#else
int64_t launch_gmm_precise(bool grad, const GmmArgs& a, hipStream_t s) {
#endif
  return grad ? launch_gmm<true>(a, s) : launch_gmm<false>(a, s);
}

#if NFN_FAST
int64_t launch_gmm_posterior_fast(const GmmArgs& a, hipStream_t s) { return launch_gmm_posterior(a, s); }
#else
int64_t launch_gmm_posterior_precise(const GmmArgs& a, hipStream_t s) { return launch_gmm_posterior(a, s); }
#endif

}  // namespace nfn
