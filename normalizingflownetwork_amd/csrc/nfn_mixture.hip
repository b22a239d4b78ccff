// nfn_mixture.hip — the kernel mixture network's density layer (GaussianKernelsLayer,
// estimators/DistributionLayers.py:74-172): log_prob of a mixture of M = n_centers *
// n_scales isotropic Gaussian kernels with per-sample logits, forward and backward.
// Compiled twice: -DNFN_FAST=1 and -DNFN_FAST=0.
//
//   c_bk   = -0.5 r2_bk / s_k^2 - d log|s_k| - 0.5 d log(2 pi),  r2_bk = sum_j (y_bj - locs_kj)^2
//   logp_b = logsumexp_k(t_bk + c_bk) - logsumexp_k(t_bk)
//
// One streaming pass over the (B, M) logits.  A G-lane group owns a row: lane l holds
// the logits k = l, l + G, ..., l + (NV - 1) G in registers (coalesced loads), the
// per-component constants sit in LDS (staged once per workgroup), and the four row
// reductions (two maxima, two sums) are DPP butterflies inside the group.  Small M packs
// 64 / G rows into a wave.  Evaluated in the shifted form
//   m_t = max_k t_k,  a'_k = (t_k - m_t) + c_k,
//   logp = max a' + log sum exp(a' - max a') - log sum exp(t - m_t),
// so no term of magnitude |t| is ever subtracted from another.
#include "nfn_launch.h"

#ifndef NFN_FAST
#error "compile with -DNFN_FAST=0 or -DNFN_FAST=1"
#endif

namespace nfn {
namespace {

constexpr bool kFast = NFN_FAST != 0;

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// G = 64: the four 16-lane rows are combined through scalar registers (four v_readlane and
// three VALU ops; no LDS round trips in the row's dependent chain of four reductions).
template <int G>
__device__ __forceinline__ float mix_gsum(float v) {
  if constexpr (G >= 64) {
    v = gsum<16>(v);
    return (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
  } else {
    return gsum<G>(v);
  }
}

// Butterfly maximum inside G-lane groups (the DPP steps of gsum).  fmaxf drops a NaN
// operand: a NaN logit reaches the result through the sums instead.
template <int G>
__device__ __forceinline__ float mix_gmax(float v) {
  if constexpr (G >= 2) v = fmaxf(v, dpp_mov<0xB1>(v));
  if constexpr (G >= 4) v = fmaxf(v, dpp_mov<0x4E>(v));
  if constexpr (G >= 8) v = fmaxf(v, dpp_mov<0x141>(v));
  if constexpr (G >= 16) v = fmaxf(v, dpp_mov<0x140>(v));
  if constexpr (G == 32) v = fmaxf(v, __shfl_xor(v, 16, 32));
  if constexpr (G >= 64)
    v = fmaxf(fmaxf(lane_value(v, 0), lane_value(v, 16)), fmaxf(lane_value(v, 32), lane_value(v, 48)));
  return v;
}

// Rows a group takes per tile: their loads are issued together (about 8 per lane in flight).
__host__ __device__ constexpr int mix_rpg(int NV) { return NV >= 8 ? 1 : 8 / NV; }

// The per-component constants, staged once per workgroup (ends on the workgroup barrier):
// [1 / s_k^2 (M) | -d log|s_k| - 0.5 d log(2 pi) (M) | 1 / s_k (M) | locs transposed (d x M)];
// 1 / s_k is written for the backward only.  The reference's bandwidth can be negative
// (include/nfn.h): |s| enters the log term only.
struct MixLds {
  const float *inv_s2, *lcs, *inv_s, *locT;
};
template <bool GRAD>
__device__ __forceinline__ MixLds mix_stage(float* lds, const MixArgs& a) {
  const int M = a.M, d = a.d, tid = threadIdx.x;
  float* inv_s2 = lds;
  float* lcs = lds + M;
  float* inv_s = lds + 2 * M;
  float* locT = lds + 3 * M;
  for (int k = tid; k < M; k += kMaxBlock) {
    const double s = (double)a.scales[k];
    inv_s2[k] = (float)(1.0 / (s * s));
    lcs[k] = (float)(-(double)d * (log(fabs(s)) + 0.91893853320467274));
    if constexpr (GRAD) inv_s[k] = (float)(1.0 / s);
  }
  for (int i = tid; i < M * d; i += kMaxBlock) {
    const int k = i / d, j = i - k * d;
    locT[j * M + k] = a.locs[i];
  }
  __syncthreads();
  return {inv_s2, lcs, inv_s, locT};
}

// Lane lg's components k = lg + G i: constant over the whole launch.  A slot past M is
// inactive and reads component 0.
template <int NV>
struct MixLane {
  int kk[NV];
  bool act[NV];
  float is2[NV], lc[NV];
};
template <int G, int NV>
__device__ __forceinline__ MixLane<NV> mix_lane(const MixLds& L, int lg, int M) {
  MixLane<NV> ln;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int k = lg + G * i;
    ln.act[i] = k < M;
    ln.kk[i] = ln.act[i] ? k : 0;
    ln.is2[i] = L.inv_s2[ln.kk[i]];
    ln.lc[i] = L.lcs[ln.kk[i]];
  }
  return ln;
}

// The kernel term of one row: z2_i = r2_i / s_i^2 and c_i = -0.5 z2_i + lc_i.  y(j) gives the
// row's raw y_j: how it is loaded is the caller's policy.
template <bool FAST, int NV, typename Y>
__device__ __forceinline__ void mix_kernel_term(const MixArgs& a, const MixLds& L, const MixLane<NV>& ln, Y y,
                                                float (&z2)[NV], float (&c)[NV]) {
  const int M = a.M;
#pragma unroll
  for (int i = 0; i < NV; ++i) z2[i] = 0.0f;
  for (int j = 0; j < a.d; ++j) {
    float yj = y(j);
    if (a.y_mean) yj = f_div<FAST>(yj - a.y_mean[j], a.y_std[j]);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const float dy = yj - L.locT[j * M + ln.kk[i]];
      z2[i] = fmaf(dy, dy, z2[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    z2[i] *= ln.is2[i];
    c[i] = fmaf(-0.5f, z2[i], ln.lc[i]);
  }
}

// One row's shifted log-sum-exp from the lane's NV logits (-inf in an inactive slot) and NV c
// values, in two steps: mt = max t, then e0 = exp(t - mt), av = (t - mt) + c, ma = max av,
// e1 = exp(av - ma), the group sums s0 and s1 of e0 and e1, and lp = (ma + log s1) - log s0 -
// corr.  The one copy of the row's formula: what a caller does not use falls away after
// inlining.  The maximum is its own step: the forward takes it as soon as the logits are
// there, before the kernel term.
template <int G, int NV>
__device__ __forceinline__ float mix_row_max(const float (&tv)[NV]) {
  float mt = tv[0];
#pragma unroll
  for (int i = 1; i < NV; ++i) mt = fmaxf(mt, tv[i]);
  return mix_gmax<G>(mt);
}
template <int G, bool FAST, int NV>
__device__ __forceinline__ void mix_row_lse(const float (&tv)[NV], const float (&c)[NV], float corr, float mt,
                                            float (&e0)[NV], float (&av)[NV], float& ma, float (&e1)[NV], float& s0,
                                            float& s1, float& lp) {
  ma = -INFINITY;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    // a lane past M and a -inf logit contribute exactly nothing (no -inf - -inf)
    const float u = tv[i] == -INFINITY ? -INFINITY : tv[i] - mt;
    e0[i] = f_exp<FAST>(u);
    av[i] = u + c[i];
    ma = fmaxf(ma, av[i]);
  }
  ma = mix_gmax<G>(ma);
  s0 = 0.0f;
  s1 = 0.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    e1[i] = av[i] == -INFINITY ? 0.0f : f_exp<FAST>(av[i] - ma);
    s0 += e0[i];
    s1 += e1[i];
  }
  s0 = mix_gsum<G>(s0);
  s1 = mix_gsum<G>(s1);
  lp = (ma + f_log<FAST>(s1)) - f_log<FAST>(s0) - corr;
}

// Forward and backward.  Loads are conditional (-inf where the row or the component is past
// the end), and a row's first y value is loaded with its logits.
template <int G, int NV, bool FAST, bool GRAD>
__global__ void __launch_bounds__(kMaxBlock) kernel_mixture_kernel(MixArgs a) {
  extern __shared__ float lds[];
  __shared__ double red[2 * kMaxBlock / 64];
  constexpr int GPB = kMaxBlock / G;  // groups per workgroup
  constexpr int RPG = mix_rpg(NV);
  constexpr int ROWS = GPB * RPG;
  const int M = a.M, d = a.d;
  const int tid = threadIdx.x;
  const MixLds L = mix_stage<GRAD>(lds, a);
  const float corr = log_std_sum<FAST>(a.y_mean, a.y_std, d);
  const int lg = tid & (G - 1), grp = tid / G;
  const MixLane<NV> ln = mix_lane<G, NV>(L, lg, M);
  [[maybe_unused]] float gs[NV];
  if constexpr (GRAD) {
#pragma unroll
    for (int i = 0; i < NV; ++i) gs[i] = 0.0f;
  }
  double acc = 0.0;
  int nfc = 0;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * ROWS + grp;
    float tv[RPG][NV];
    float y0[RPG];  // the rows' first y value, loaded with the logits (d = 1: all of y)
    [[maybe_unused]] float g0[RPG];
#pragma unroll
    for (int r = 0; r < RPG; ++r) {
      const int64_t b = b0 + (int64_t)r * GPB;
      const float* tr = a.logits + b * a.rs;
      y0[r] = a.y[b < a.B ? b * a.y_bstride : 0];
      if constexpr (GRAD) g0[r] = b < a.B ? (a.g_out ? a.g_out[b] : 1.0f) : 0.0f;
#pragma unroll
      for (int i = 0; i < NV; ++i)
        tv[r][i] = (b < a.B && ln.act[i]) ? __builtin_nontemporal_load(tr + lg + G * i) : -INFINITY;
    }
#pragma unroll
    for (int r = 0; r < RPG; ++r) {
      const int64_t b = b0 + (int64_t)r * GPB;
      const bool ok = b < a.B;
      const float* yr = a.y + (ok ? b * a.y_bstride : 0);
      float z2[NV], c[NV], av[NV], e0[NV], e1[NV];
      float ma, s0, s1, lp;
      const float mt = mix_row_max<G>(tv[r]);
      const auto y = [&](int j) { return j == 0 ? y0[r] : yr[j]; };
      mix_kernel_term<FAST>(a, L, ln, y, z2, c);
      mix_row_lse<G, FAST>(tv[r], c, corr, mt, e0, av, ma, e1, s0, s1, lp);
      if (ok && lg == 0) {
        if (a.out) a.out[b] = lp;
        acc += (double)lp;
        nfc += nonfinite1(lp);
      }
      if constexpr (GRAD) {
        const float g = g0[r];
        const float r0 = f_div<FAST>(1.0f, s0), r1 = f_div<FAST>(1.0f, s1);
        float post[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          post[i] = e1[i] * r1;
          if (ok && ln.act[i]) {
            if (a.grad_logits)
              __builtin_nontemporal_store(g * (post[i] - e0[i] * r0), a.grad_logits + b * a.gl_rs + lg + G * i);
            // d/ds_k: post (r2 / s^3 - d / s) = post (z2 - d) / s
            gs[i] = fmaf(g * post[i], (z2[i] - (float)d) * L.inv_s[ln.kk[i]], gs[i]);
          }
        }
        if (a.grad_y) {
          for (int j = 0; j < d; ++j) {
            float yj = y(j);
            float sd = 1.0f;
            if (a.y_mean) {
              sd = a.y_std[j];
              yj = f_div<FAST>(yj - a.y_mean[j], sd);
            }
            float p = 0.0f;
#pragma unroll
            for (int i = 0; i < NV; ++i) p = fmaf(post[i] * ln.is2[i], L.locT[j * M + ln.kk[i]] - yj, p);
            p = mix_gsum<G>(p);
            if (ok && lg == 0) a.grad_y[b * d + j] = a.y_mean ? f_div<FAST>(g * p, sd) : g * p;
          }
        }
      }
    }
  }
  if constexpr (GRAD) {
    if (a.part) {
      // grad_scales: the groups' accumulators summed in group order, one partial row per
      // workgroup (finished in fixed order by sum_partials_kernel): bitwise deterministic
      __syncthreads();  // the staged constants are dead
#pragma unroll
      for (int i = 0; i < NV; ++i) lds[i * kMaxBlock + tid] = gs[i];
      __syncthreads();
      for (int k = tid; k < M; k += kMaxBlock) {
        const int i = k / G, l = k - i * G;
        float s = 0.0f;
        for (int q = 0; q < GPB; ++q) s += lds[i * kMaxBlock + q * G + l];
        a.part[(int64_t)blockIdx.x * M + k] = s;
      }
    }
  } else {
    if (a.partials) write_partial(a.partials, acc, nfc, red, a.out_sum, a.epoch);
  }
}

// The posterior score (BayesianNNEstimator.score, BayesianNNEstimator.py:65-76) of the same
// layer: logsumexp over a.nd draws of the row's log_prob, minus log S, on the forward's
// (G, NV) groups and tiles.  c_bk depends on y_b and the centres only, so a row's NV values
// per lane are formed once (mix_kernel_term) and kept in registers; per draw only the NV
// logits are loaded, and the next draw's loads are issued before this draw's reductions.
// Each draw's log_prob is the forward's mix_row_lse.
template <int G, int NV, bool FAST>
__global__ void __launch_bounds__(kMaxBlock) kernel_mixture_posterior_kernel(MixArgs a) {
  extern __shared__ float lds[];
  __shared__ double red[2 * kMaxBlock / 64];
  constexpr int GPB = kMaxBlock / G;  // groups per workgroup
  constexpr int RPG = mix_rpg(NV);
  constexpr int ROWS = GPB * RPG;
  const int S = a.nd;
  const int tid = threadIdx.x;
  const MixLds L = mix_stage<false>(lds, a);
  const float corr = log_std_sum<FAST>(a.y_mean, a.y_std, a.d);
  const int lg = tid & (G - 1), grp = tid / G;
  const MixLane<NV> ln = mix_lane<G, NV>(L, lg, a.M);
  double acc = 0.0;
  int nfc = 0;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * ROWS + grp;
    // The next draw's logits, in flight.  Every load is unconditional, from a clamped address
    // (row 0 past B, column 0 past M), and masked when it is consumed: a load under a per-lane
    // condition is waited for where its branch joins, one memory latency after the other.
    float nx[RPG][NV];
    const float* tr[RPG];
#pragma unroll
    for (int r = 0; r < RPG; ++r) {
      const int64_t b = b0 + (int64_t)r * GPB;
      tr[r] = a.logits + (b < a.B ? b : 0) * a.rs;
#pragma unroll
      for (int i = 0; i < NV; ++i) nx[r][i] = __builtin_nontemporal_load(tr[r] + ln.kk[i]);
    }
    // the S-independent part: c_k of every row of the tile
    float cv[RPG][NV];
#pragma unroll
    for (int r = 0; r < RPG; ++r) {
      const int64_t b = b0 + (int64_t)r * GPB;
      const float* yr = a.y + (b < a.B ? b * a.y_bstride : 0);
      float z2[NV];
      mix_kernel_term<FAST>(a, L, ln, [&](int j) { return yr[j]; }, z2, cv[r]);
    }
    float m[RPG], la[RPG];
#pragma unroll
    for (int r = 0; r < RPG; ++r) {
      m[r] = -INFINITY;
      la[r] = 0.0f;
    }
    for (int s = 0; s < S; ++s) {
      float tv[RPG][NV];
#pragma unroll
      for (int r = 0; r < RPG; ++r) {
        const bool ok = b0 + (int64_t)r * GPB < a.B;
#pragma unroll
        for (int i = 0; i < NV; ++i) tv[r][i] = (ok && ln.act[i]) ? nx[r][i] : -INFINITY;
      }
      if (s + 1 < S) {
#pragma unroll
        for (int r = 0; r < RPG; ++r) {
          const float* tn = tr[r] + (int64_t)(s + 1) * a.ds;
#pragma unroll
          for (int i = 0; i < NV; ++i) nx[r][i] = __builtin_nontemporal_load(tn + ln.kk[i]);
        }
      }
#pragma unroll
      for (int r = 0; r < RPG; ++r) {
        float av[NV], e0[NV], e1[NV];
        float ma, s0, s1, lp;
        mix_row_lse<G, FAST>(tv[r], cv[r], corr, mix_row_max<G>(tv[r]), e0, av, ma, e1, s0, s1, lp);
        // every logit -inf (s0 is exactly 0 then, and only then): the draw has no component
        // left, its term is -inf and drops out (the single-draw entry gives NaN, -inf - -inf)
        lp = s0 == 0.0f ? -INFINITY : lp;
        lse_push<FAST>(m[r], la[r], lp);
      }
    }
#pragma unroll
    for (int r = 0; r < RPG; ++r) {
      const int64_t b = b0 + (int64_t)r * GPB;
      if (b < a.B && lg == 0) {
        const float res = lse_finish<FAST>(m[r], la[r], S);
        if (a.out) a.out[b] = res;
        acc += (double)res;
        nfc += nonfinite1(res);
      }
    }
  }
  if (a.partials) write_partial(a.partials, acc, nfc, red, a.out_sum, a.epoch);
}

// The (G, NV) instance for M components, handed to f as compile-time constants.  The row
// reductions cost the same wave instructions whatever G is, so the narrowest group whose
// lanes can hold the row (<= 16 values each) is the cheapest per row: up to M = 256 a
// 16-lane group (DPP only, four rows per wave), then 32 and 64 lanes.
template <int G_, int NV_>
struct MixShape {
  static constexpr int G = G_, NV = NV_;
};
template <typename F>
int64_t for_mix_shape(int M, F f) {
  if (M <= 1) return f(MixShape<1, 1>{});
  if (M <= 2) return f(MixShape<2, 1>{});
  if (M <= 4) return f(MixShape<4, 1>{});
  if (M <= 8) return f(MixShape<8, 1>{});
  if (M <= 16) return f(MixShape<16, 1>{});
  if (M <= 32) return f(MixShape<16, 2>{});
  if (M <= 64) return f(MixShape<16, 4>{});
  if (M <= 128) return f(MixShape<16, 8>{});
  if (M <= 256) return f(MixShape<16, 16>{});
  if (M <= 512) return f(MixShape<32, 16>{});
  if (M <= 1024) return f(MixShape<64, 16>{});
  return 0;
}

template <int G, int NV, typename KFN>
int64_t launch_one(KFN kfn, const MixArgs& a0, size_t lds, hipStream_t s) {
  MixArgs a = a0;
  constexpr int ROWS = (kMaxBlock / G) * mix_rpg(NV);
  a.ntiles = (a.B + ROWS - 1) / ROWS;
  int64_t grid = persistent_grid(kfn, kMaxBlock, lds, a.ntiles);
  grid = std::max<int64_t>(1, std::min(grid, a.grid_cap));
  nfn_launch(kfn, dim3((unsigned)grid), dim3(kMaxBlock), (uint32_t)lds, s, a);
  return grid;
}

template <bool GRAD>
int64_t launch_shape(const MixArgs& a, size_t lds, hipStream_t s) {
  return for_mix_shape(a.M, [&](auto sh) {
    constexpr int G = decltype(sh)::G, NV = decltype(sh)::NV;
    // the grad_scales hand-over reuses the LDS
    const size_t need = GRAD ? std::max(lds, sizeof(float) * NV * kMaxBlock) : lds;
    return launch_one<G, NV>(kernel_mixture_kernel<G, NV, kFast, GRAD>, a, need, s);
  });
}

}  // namespace

#if NFN_FAST
int64_t launch_mixture_fast(bool grad, const MixArgs& a, size_t lds, hipStream_t s) {
#else
int64_t launch_mixture_precise(bool grad, const MixArgs& a, size_t lds, hipStream_t s) {
#endif
  return grad ? launch_shape<true>(a, lds, s) : launch_shape<false>(a, lds, s);
}

#if NFN_FAST
int64_t launch_mixture_posterior_fast(const MixArgs& a, size_t lds, hipStream_t s) {
#else
int64_t launch_mixture_posterior_precise(const MixArgs& a, size_t lds, hipStream_t s) {
#endif
  return for_mix_shape(a.M, [&](auto sh) {
    constexpr int G = decltype(sh)::G, NV = decltype(sh)::NV;
    return launch_one<G, NV>(kernel_mixture_posterior_kernel<G, NV, kFast>, a, lds, s);
  });
}

}  // namespace nfn
