// nfn_dense_device.h — the pieces of the fused Dense kernels' tile pipeline (nfn_dense.hip,
// nfn_dense_grad.hip) as forced-inline helpers.  The kernels that call them keep their loops,
// their waits and their wave_lds_sync placement.  Callers: chain_dense1_kernel and
// chain_dense1_grad_sb_kernel throughout, chain_dense1_grad_kernel for the memory side; the
// other five kernels write the same pipeline in their own text (below, and DESIGN.md).
//
// A wave owns a stream of 64-sample tiles.  Per tile (per (tile, draw) unit in the posterior):
//   span      the tile's rows [b0, b0 + nr) and the buffer descriptors bounded at them
//             (loads past B return 0, stores past B are dropped: no branch on the last tile);
//   prefetch  the NEXT tile's h rows (and the posterior's W_s / bias fragments) into
//             registers while this tile computes; at the hand-off they go to the wave's LDS
//             slot, to be read back as MFMA A fragments;
//   t GEMM    t = h W + b with v_mfma_f32_16x16x4_f32 (exact fp32): lane (am, ak) =
//             (lane % 16, lane / 16) supplies A[row 16 mt + am][k = 4 ks + ak] and
//             B[k = 4 ks + ak][column 16 nt + am], and receives C[rows 16 mt + 4 ak .. + 3][column
//             16 nt + am]; k-steps outer, the four M tiles inner, accumulators from zero;
//   t tile    the accumulators + bias go to the wave's t tile, column-major at kCS (b128
//             stores, the d = 1 kernels) or row-major at an odd stride (the d-general ones);
//   chain     per lane, one sample; the d = 1 forward and backward pick the chain form here;
//   store     the forward's result leaves one tile late (PendingOut), the backward's
//             log_prob and dy at once.
// The B operand and the bias value come from the caller (registers, LDS, global memory).
// The three synchronous kernels (chain_dense_kernel, posterior_dense_kernel,
// chain_dense_grad_kernel: plain pointers, H a run-time value) write the same GEMM as
// run-time loops in their own text: with these helpers their register allocation moved.
// The two prefetching posterior kernels and chain_dense1_grad_kernel's compute side keep their
// own text too: with the helpers they measured a few tenths of a percent slower than before
// ("Fused Dense kernels: shared pipeline pieces").
#pragma once

#include "nfn_bf16.h"
#include "nfn_grad_device.h"
#include "nfn_launch.h"

namespace nfn {

constexpr int kDenseNT = 2;  // cache policy of the h loads and the result stores: non-temporal

// ---- tile span ------------------------------------------------------------------------
struct TileSpan {
  int64_t b0;   // first row
  int64_t nr;   // rows in [0, 64]: tiles past the end are empty
  int64_t b0c;  // b0, or 0 for an empty tile (descriptor bases stay inside the tensors)
};
__device__ __forceinline__ TileSpan tile_span(int64_t tile, int64_t B) {
  const int64_t b0 = tile * 64;
  const int64_t nr = max((int64_t)0, min((int64_t)64, B - b0));
  return {b0, nr, nr > 0 ? b0 : 0};
}
// the tile's y rows (d values each)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_y(const ChainArgs& a, const TileSpan& sp, int d) {
  return tile_rsrc(a.y + sp.b0c * a.y_bstride, sp.nr > 0 ? ((sp.nr - 1) * a.y_bstride + d) * 4 : 0);
}
// the tile's h rows (H values each) of draw sd
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_h(const DenseArgs& da, const TileSpan& sp, int H, int sd = 0) {
  const int64_t hs = da.h_rowstride;
  return tile_rsrc(da.h + sd * da.h_drawstride + sp.b0c * hs, sp.nr > 0 ? ((sp.nr - 1) * hs + H) * 4 : 0);
}
// the tile's upstream gradients (without g_out: an empty descriptor, the value is replaced by 1)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_g(const DenseGradArgs& g, const TileSpan& sp) {
  return tile_rsrc(g.g_out ? g.g_out + sp.b0c : g.da.c.y, g.g_out ? sp.nr * 4 : 0);
}
// one float per row of an optional output (out, grad_y); NULL: empty
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_out(float* p, const TileSpan& sp) {
  return tile_rsrc(p && sp.nr > 0 ? p + sp.b0 : p, p ? sp.nr * 4 : 0);
}
// H floats per row of grad_h (row stride ghs); NULL: empty
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_grad_h(const DenseGradArgs& g, const TileSpan& sp, int H) {
  const int64_t ghs = g.gh_rowstride;
  return tile_rsrc(g.grad_h && sp.nr > 0 ? g.grad_h + sp.b0 * ghs : g.grad_h,
                   g.grad_h && sp.nr > 0 ? ((sp.nr - 1) * ghs + H) * 4 : 0);
}
__device__ __forceinline__ float load_f32(__amdgpu_buffer_rsrc_t r, int off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}

// ---- h prefetch and hand-off ----------------------------------------------------------
// Forward / posterior: lane (r0, c4) = (lane / QH, lane % QH) holds float4 c4 of the rows
// r0 + k RSTEP (RSTEP = 64 / QH): hoff = its byte offset in the tile, kstep = RSTEP rows.
template <int QH>
__device__ __forceinline__ void load_h_rows(float4 (&buf)[QH], __amdgpu_buffer_rsrc_t rh, int hoff, int kstep) {
#pragma unroll
  for (int k = 0; k < QH; ++k)
    buf[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rh, hoff, k * kstep, kDenseNT));
}
// dst = hl + r0 SH + 4 c4, rowstep = RSTEP SH
template <int QH>
__device__ __forceinline__ void store_h_rows(float* dst0, int rowstep, const float4 (&buf)[QH]) {
#pragma unroll
  for (int k = 0; k < QH; ++k) {
    float* dst = dst0 + k * rowstep;
    dst[0] = buf[k].x;
    dst[1] = buf[k].y;
    dst[2] = buf[k].z;
    dst[3] = buf[k].w;
  }
}
// Backward (d = 1): lane (am, ak) holds h[16 mt + am][16 j + 4 ak .. + 3]; hoff = its byte
// offset in the tile, hmt = 16 rows; LDS rows at SH = H + 4 (conflict-free b128 writes).
template <int MH>
__device__ __forceinline__ void load_h_frags(float4 (&hb)[4][MH], __amdgpu_buffer_rsrc_t rh, int hoff, int hmt) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < MH; ++j)
      hb[mt][j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rh, hoff, mt * hmt + 64 * j, kDenseNT));
}
template <int MH>
__device__ __forceinline__ void store_h_frags(float* hl, int SH, int am, int ak, const float4 (&hb)[4][MH]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int j = 0; j < MH; ++j) *reinterpret_cast<float4*>(hl + (16 * mt + am) * SH + 16 * j + 4 * ak) = hb[mt][j];
}
// The d = 1 backward kernels' prefetch of one tile: y, the upstream gradient, the h rows.
template <int MH>
__device__ __forceinline__ void dense1_grad_issue(const DenseGradArgs& g, int64_t tile, int64_t u0, int lane, int yoff,
                                                  int hoff, int hmt, float& ybuf, float& gbuf, float4 (&hb)[4][MH]) {
  const ChainArgs& a = g.da.c;
  if (diag_ablate_loads(a)) tile = u0;  // diagnostic: compute-only timing (the first tile re-read)
  const TileSpan sp = tile_span(tile, a.B);
  ybuf = load_f32(span_y(a, sp, 1), yoff);
  gbuf = load_f32(span_g(g, sp), lane * 4);
  load_h_frags<MH>(hb, span_h(g.da, sp, 16 * MH), hoff, hmt);
}

// ---- the f32 t GEMM -------------------------------------------------------------------
__device__ __forceinline__ void zero_acc(f32x4v (&acc)[4]) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
}
// the tile's A fragments (4 M tiles x QH k-steps), read once for every N tile
template <int QH>
__device__ __forceinline__ void read_a_frags(float (&av)[4][QH], const float* hl, int SH, int am, int ak) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int ks = 0; ks < QH; ++ks) av[mt][ks] = hl[(16 * mt + am) * SH + 4 * ks + ak];
}
// one N tile: acc = h W[:, 16 nt .. 16 nt + 15], bfrag(ks) = this lane's B value of k-step ks
template <int QH, class BFrag>
__device__ __forceinline__ void t_ntile(f32x4v (&acc)[4], const float (&av)[4][QH], BFrag bfrag) {
  zero_acc(acc);
#pragma unroll
  for (int ks = 0; ks < QH; ++ks) {
    const float bv = bfrag(ks);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][ks], bv, acc[mt], 0, 0, 0);
  }
}
// column n of t, column-major at kCS: rows 16 mt + 4 ak .. + 3 as one b128 (n < P: the caller's guard)
__device__ __forceinline__ void store_t_cols(float* tl, int n, int ak, const f32x4v (&acc)[4], float bn) {
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<f32x4v*>(tl + n * kCS + 16 * mt + 4 * ak) = acc[mt] + bn;
}

// ---- d = 1 y normalisation ------------------------------------------------------------
struct Norm1 {
  bool on;
  float mean, std, corr;  // corr = log std, subtracted from log_prob
};
__device__ __forceinline__ Norm1 norm1(const ChainArgs& a) {
  Norm1 n{a.y_mean != nullptr, 0.0f, 1.0f, 0.0f};
  if (n.on) {
    n.mean = a.y_mean[0];
    n.std = a.y_std[0];
    n.corr = f_log<true>(n.std);
  }
  return n;
}
__device__ __forceinline__ float norm1_z(const Norm1& n, float y) { return n.on ? f_div<true>(y - n.mean, n.std) : y; }
__device__ __forceinline__ float norm1_dy(const Norm1& n, float adj) { return n.on ? f_div<true>(adj, n.std) : adj; }

// ---- chain dispatch (d = 1, t column-major at kCS, col = tl + lane) --------------------
template <int CM>
__device__ __forceinline__ float dense1_chain(float z0, const float* col, const ChainArgs& a) {
  return a.prog.K <= 16 ? eval_chain1_fast<true, kCS, CM, false>(z0, col, a)
                        : eval_chain1_fast<false, kCS, kChainLoop, false>(z0, col, a);
}
// The programs the fused Dense backward runs as compile-time blocks with the parameter-scalar
// cache (SP indexes them): C2's (planar, radial) x 5, and the estimator's default
// NormalizingFlowNetwork(n_dims, n_flows=10), radial x 10 (NormalizingFlowNetwork.py:10-17).
constexpr uint32_t kCacheTypes[] = {0x44444u, 0x55555u};
constexpr int kCacheK[] = {10, 10};
constexpr int kNumCached = 2;
// forward + reverse: the lane's t column becomes g * d logp / d t; returns log_prob (before
// the normalisation's correction), adj = d logp / d z_0
template <int CM, int SP = 0>
__device__ __forceinline__ float dense1_grad_chain(float& z, float* col, float* zh, const ChainArgs& a, float gl,
                                                   float& adj) {
  const int K = a.prog.K, P = a.P;
  const bool trainable = a.trainable != 0, want = a.out != nullptr;
  const uint32_t types = a.prog.types[0];
  if constexpr (CM == kStaticCache || CM == kStaticCacheX)
    return grad1_static_cache<kCacheTypes[SP], kCacheK[SP], kCS, CM == kStaticCache>(z, col, P, trainable, gl, want, adj);
  else if constexpr (CM == kStaticProg)
    return grad1_static<kStaticTypes[0], kStaticK[0], kCS>(z, col, zh, 64, P, trainable, gl, want, adj);
  else if constexpr (CM >= kChainHPair && (CM - kChainHPair) / 9 == 2)  // flow inputs in registers
    return grad1_hpairs_regs<((CM - kChainHPair) % 9) / 3, (CM - kChainHPair) % 3, kCS>(z, col, K, P, trainable, gl, want,
                                                                                         adj);
  else if constexpr (CM >= kChainHPair)
    return grad1_hpairs<((CM - kChainHPair) % 9) / 3, (CM - kChainHPair) % 3, kCS>(z, col, zh, 64, K, P, trainable, gl,
                                                                                   want, adj);
  else if constexpr (CM == kChainPairs)
    return grad1_pairs<kCS>(z, col, zh, 64, types, K, P, trainable, gl, want, adj);
  else
    return grad1_packed<kCS>(z, col, zh, 64, types, K, P, trainable, gl, want, adj);
}

// ---- result stores --------------------------------------------------------------------
// The forward's log_prob / score of a tile, stored after the NEXT prefetch has been issued
// (every path into the loop ends [loads][store]: counted waits); an empty descriptor stores
// nothing.
struct PendingOut {
  __amdgpu_buffer_rsrc_t r;
  float v;
};
__device__ __forceinline__ PendingOut pend_none(const ChainArgs& a) { return {tile_rsrc(a.out, 0), 0.0f}; }
__device__ __forceinline__ void pend_flush(const PendingOut& p, int lane) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, p.v), p.r, lane * 4, 0, kDenseNT);
}
__device__ __forceinline__ void pend_set(PendingOut& p, const ChainArgs& a, const TileSpan& sp, float v) {
  p.v = v;
  p.r = span_out(a.out, sp);
}
// the backward's log_prob and dy of a tile
__device__ __forceinline__ void store_lp_grad_y(const DenseGradArgs& g, const TileSpan& sp, int lane, float lp, float gy) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, lp), span_out(g.da.c.out, sp), lane * 4, 0, kDenseNT);
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, gy), span_out(g.grad_y, sp), lane * 4, 0, kDenseNT);
}
// rows past B carry no gradient: their dt entries (column-major tile) are zeroed
__device__ __forceinline__ void zero_dt_past_B(float* tl, int P, int64_t nr, int lane) {
  if (nr < 64 && lane >= nr) {
    for (int p = 0; p < P; ++p) tl[p * kCS + lane] = 0.0f;
  }
}

}  // namespace nfn
