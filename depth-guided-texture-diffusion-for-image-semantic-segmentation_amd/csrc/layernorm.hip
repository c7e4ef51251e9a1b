// layernorm.hip — LayerNorm over the channel dim of a [rows, C] token matrix (fwd + bwd).
// Replaces nn.LayerNorm / F.layer_norm of twig/model/cod.py:979, 881, 929, 936, 1367-1391, 1043.
//
// HBM-bound: algorithmic bytes fwd = 2*e*rows*C, bwd = 3*e*rows*C (e = element size).
// Mapping: a row is cut into 16-byte chunks; a power-of-two group of G lanes owns one row
// (64/G rows per wave), every lane keeps its chunks in registers, moments are reduced inside
// the group in registers (group_sum<G>, common.h).  No LDS in the forward.
//
// Most launches of the model are a single trip of a single wave of workgroups, so a launch lasts as long as the dependent chain
// of one wave.  The kernels keep that chain short: every global load of a trip (gamma/beta, then the rows) is issued before the first
// wait and none stands under a branch (idle lanes and the rows past the end load from a clamped address and select zero), the
// reductions of all U rows and of both sums advance together, and the rows are stored after the last of them.
#include "common.h"

namespace {

constexpr int LN_MAX_NPL = 4;      // chunks per lane: covers C <= 1024 (fp32) / 2048 (bf16)
constexpr int LN_BWD_MAX_GRID = 1024;
constexpr int ln_rows_in_flight(int npl) { return npl <= 2 ? 4 : 2; }   // U: rows per lane group and trip

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte load of a parameter vector that is only 4-byte aligned

// which chunks of a row a lane owns: chunk gl + i*G for i < NPL; lanes past the row's end point at the last chunk and hold zeros
template <typename T, int NPL, int G>
struct LnLane {
  static constexpr int V = Vec16<T>::N;
  bool in[NPL];
  int off[NPL];   // element offset of chunk i inside a row, clamped
  __device__ __forceinline__ LnLane(int gl, int cpr) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) { const int c = gl + i * G; in[i] = c < cpr; off[i] = (in[i] ? c : cpr - 1) * V; }
  }
  // the lane's columns of a per-column fp32 vector, zero in idle lanes
  __device__ __forceinline__ void load_param(const float* __restrict__ p, float (&o)[NPL][V]) const {
    f32x4 t[NPL][V / 4];
#pragma unroll
    for (int i = 0; i < NPL; ++i)
#pragma unroll
      for (int k = 0; k < V / 4; ++k) t[i][k] = *reinterpret_cast<const f32x4_a4*>(p + off[i] + 4 * k);
#pragma unroll
    for (int i = 0; i < NPL; ++i)
#pragma unroll
      for (int j = 0; j < V; ++j) o[i][j] = in[i] ? t[i][j / 4][j % 4] : 0.f;
  }
};

template <typename T, int NPL, int G>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, T* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     int64_t rows, int C, float eps) {
  typedef typename Vec16<T>::type VT;
  constexpr int V = Vec16<T>::N, U = ln_rows_in_flight(NPL), RPW = 64 / G, RPB = RPW * 4;   // rows per wave / per workgroup and u
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane & (G - 1), gi = lane / G;
  const float invC = 1.f / (float)C;
  const LnLane<T, NPL, G> ll(gl, C / V);
  // per-lane gamma/beta (column mapping is row-independent)
  float gm[NPL][V], bt[NPL][V];
  ll.load_param(gamma, gm);
  ll.load_param(beta, bt);
  for (int64_t r0 = (int64_t)blockIdx.x * RPB * U; r0 < rows; r0 += (int64_t)gridDim.x * RPB * U) {
    VT t[U][NPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r0 + u * RPB + wave * RPW + gi, row = rr < rows ? rr : rows - 1;
#pragma unroll
      for (int i = 0; i < NPL; ++i) t[u][i] = *reinterpret_cast<const VT*>(x + row * C + ll.off[i]);
    }
    float v[U][NPL][V], s[U], q[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s[u] = 0.f;
#pragma unroll
      for (int i = 0; i < NPL; ++i)
#pragma unroll
        for (int j = 0; j < V; ++j) { v[u][i][j] = ll.in[i] ? (float)t[u][i][j] : 0.f; s[u] += v[u][i][j]; }
    }
    group_sum<G>(s);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s[u] *= invC;   // mean
      q[u] = 0.f;
#pragma unroll
      for (int i = 0; i < NPL; ++i)
#pragma unroll
        for (int j = 0; j < V; ++j) { float d = ll.in[i] ? v[u][i][j] - s[u] : 0.f; q[u] = __builtin_fmaf(d, d, q[u]); }
    }
    group_sum<G>(q);
    // every row's outputs come from the ONE copy of the arithmetic below (with its multiply-adds spelled out: which of them fuse is
    // not left to the compiler, so a row's bits do not depend on its slot u); the workgroup-uniform branch after it only stores
    VT o[U][NPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      q[u] = rsqrtf(__builtin_fmaf(q[u], invC, eps));
#pragma unroll
      for (int i = 0; i < NPL; ++i)
#pragma unroll
        for (int j = 0; j < V; ++j) o[u][i][j] = (T)__builtin_fmaf((v[u][i][j] - s[u]) * q[u], gm[i][j], bt[i][j]);
    }
    auto store_row = [&](int u, int64_t row) {
#pragma unroll
      for (int i = 0; i < NPL; ++i)
        if (ll.in[i]) *reinterpret_cast<VT*>(y + row * C + ll.off[i]) = o[u][i];
      if (gl == 0) { mean[row] = s[u]; rstd[row] = q[u]; }
    };
    const int64_t first = r0 + wave * RPW + gi;
    if (r0 + (int64_t)RPB * U <= rows) {       // workgroup-uniform: every row of the trip exists
#pragma unroll
      for (int u = 0; u < U; ++u) store_row(u, first + u * RPB);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (first + u * RPB < rows) store_row(u, first + u * RPB);
    }
  }
}

// Backward: dx per row; per-block partial dgamma/dbeta written to ws[block][2][C].
template <typename T, int NPL, int G>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const T* __restrict__ dres, T* __restrict__ dx,
                                                     float* __restrict__ ws, int64_t rows, int C) {
  typedef typename Vec16<T>::type VT;
  constexpr int V = Vec16<T>::N, U = ln_rows_in_flight(NPL), RPW = 64 / G, RPB = RPW * 4;
  extern __shared__ float red[];  // [4 waves][2][C]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int gl = lane & (G - 1), gi = lane / G;
  const float invC = 1.f / (float)C;
  const LnLane<T, NPL, G> ll(gl, C / V);
  float gm[NPL][V], dg[NPL][V], db[NPL][V];
#pragma unroll
  for (int i = 0; i < NPL; ++i)
#pragma unroll
    for (int j = 0; j < V; ++j) { dg[i][j] = 0.f; db[i][j] = 0.f; }
  ll.load_param(gamma, gm);
  for (int64_t r0 = (int64_t)blockIdx.x * RPB * U; r0 < rows; r0 += (int64_t)gridDim.x * RPB * U) {
    VT tx[U][NPL], tg[U][NPL], tr[U][NPL];
    float mu[U], rs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t rr = r0 + u * RPB + wave * RPW + gi, row = rr < rows ? rr : rows - 1;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        tx[u][i] = *reinterpret_cast<const VT*>(x + row * C + ll.off[i]);
        tg[u][i] = *reinterpret_cast<const VT*>(dy + row * C + ll.off[i]);
      }
      mu[u] = mean[row]; rs[u] = rstd[row];
    }
    if (dres) {      // gradient of the residual branch that forks off x (kernel-uniform)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t rr = r0 + u * RPB + wave * RPW + gi, row = rr < rows ? rr : rows - 1;
#pragma unroll
        for (int i = 0; i < NPL; ++i) tr[u][i] = *reinterpret_cast<const VT*>(dres + row * C + ll.off[i]);
      }
    }
    const int64_t first = r0 + wave * RPW + gi;
    const bool full = r0 + (int64_t)RPB * U <= rows;     // workgroup-uniform: every row of the trip exists
    float xv[U][NPL][V], gv[U][NPL][V], ab[2 * U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = full || first + u * RPB < rows;    // a row past the end adds zeros to dgamma/dbeta
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int i = 0; i < NPL; ++i) {
        const bool in = ll.in[i] && ok;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          float xh = in ? ((float)tx[u][i][j] - mu[u]) * rs[u] : 0.f;
          float g = in ? (float)tg[u][i][j] : 0.f;
          dg[i][j] = __builtin_fmaf(g, xh, dg[i][j]);
          db[i][j] += g;
          g *= gm[i][j];
          a += g; b = __builtin_fmaf(g, xh, b);
          xv[u][i][j] = xh; gv[u][i][j] = g;
        }
      }
      ab[2 * u] = a; ab[2 * u + 1] = b;
    }
    group_sum<G>(ab);
    // every row's dx comes from the ONE copy of the arithmetic below, multiply-adds spelled out (see the forward); the
    // workgroup-uniform branch after it only stores
    VT o[U][NPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float a = ab[2 * u] * invC, b = ab[2 * u + 1] * invC;
#pragma unroll
      for (int i = 0; i < NPL; ++i)
#pragma unroll
        for (int j = 0; j < V; ++j)
          o[u][i][j] = (T)__builtin_fmaf(rs[u], __builtin_fmaf(-xv[u][i][j], b, gv[u][i][j] - a), dres ? (float)tr[u][i][j] : 0.f);
    }
    auto store_row = [&](int u, int64_t row) {
#pragma unroll
      for (int i = 0; i < NPL; ++i)
        if (ll.in[i]) *reinterpret_cast<VT*>(dx + row * C + ll.off[i]) = o[u][i];
    };
    if (full) {
#pragma unroll
      for (int u = 0; u < U; ++u) store_row(u, first + u * RPB);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (first + u * RPB < rows) store_row(u, first + u * RPB);
    }
  }
  // combine the 64/G row-groups of the wave (same column set), then the 4 waves through LDS
#pragma unroll
  for (int i = 0; i < NPL; ++i) {
    if constexpr (G <= 1)  { lane_xor_add<1>(dg[i]);  lane_xor_add<1>(db[i]); }
    if constexpr (G <= 2)  { lane_xor_add<2>(dg[i]);  lane_xor_add<2>(db[i]); }
    if constexpr (G <= 4)  { lane_xor_add<4>(dg[i]);  lane_xor_add<4>(db[i]); }
    if constexpr (G <= 8)  { lane_xor_add<8>(dg[i]);  lane_xor_add<8>(db[i]); }
    if constexpr (G <= 16) { lane_xor_add<16>(dg[i]); lane_xor_add<16>(db[i]); }
    if constexpr (G <= 32) { lane_xor_add<32>(dg[i]); lane_xor_add<32>(db[i]); }
  }
  if (gi == 0) {
#pragma unroll
    for (int i = 0; i < NPL; ++i) {
      if (ll.in[i])
#pragma unroll
        for (int j = 0; j < V; ++j) { red[(wave * 2 + 0) * C + ll.off[i] + j] = dg[i][j]; red[(wave * 2 + 1) * C + ll.off[i] + j] = db[i][j]; }
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * C; c += 256) {
    int which = c / C, col = c % C;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) s += red[(w * 2 + which) * C + col];
    ws[((size_t)blockIdx.x * 2 + which) * C + col] = s;
  }
}

struct LnGeom { int G, npl; int64_t rows_per_block; };
template <typename T> LnGeom ln_geom(int C) {
  int cpr = C / Vec16<T>::N;
  int G = 1;
  while (G < cpr && G < 64) G <<= 1;
  LnGeom g; g.G = G; g.npl = (cpr + G - 1) / G; g.rows_per_block = (64 / G) * 4;
  return g;
}

// run STMT with NPL_ / G_ bound to the geometry: more than one chunk per lane occurs only with full-wave groups
#define LN_DISPATCH(g, STMT) do { \
    if ((g).G == 64) { constexpr int G_ = 64; \
      if ((g).npl == 1) { constexpr int NPL_ = 1; STMT; } else if ((g).npl == 2) { constexpr int NPL_ = 2; STMT; } \
      else if ((g).npl == 3) { constexpr int NPL_ = 3; STMT; } else { constexpr int NPL_ = 4; STMT; } } \
    else { constexpr int NPL_ = 1; \
      if ((g).G == 32) { constexpr int G_ = 32; STMT; } else if ((g).G == 16) { constexpr int G_ = 16; STMT; } \
      else if ((g).G == 8) { constexpr int G_ = 8; STMT; } else if ((g).G == 4) { constexpr int G_ = 4; STMT; } \
      else if ((g).G == 2) { constexpr int G_ = 2; STMT; } else { constexpr int G_ = 1; STMT; } } } while (0)

template <typename T>
int ln_fwd_launch(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                  int64_t rows, int C, float eps, hipStream_t s) {
  DGTD_REQUIRE(C % Vec16<T>::N == 0, "layernorm: C=%d must be a multiple of %d", C, Vec16<T>::N);
  LnGeom g = ln_geom<T>(C);
  DGTD_REQUIRE(g.npl <= LN_MAX_NPL, "layernorm: C=%d too large", C);
  if (rows == 0) return 0;
  int grid = (int)std::min<int64_t>(cdiv(rows, g.rows_per_block * ln_rows_in_flight(g.npl)), 256 * 8);
  LN_DISPATCH(g, hipLaunchKernelGGL((ln_fwd_kernel<T, NPL_, G_>), dim3(grid), dim3(256), 0, s, (const T*)x, gamma, beta, (T*)y, mean, rstd, rows, C, eps));
  DGTD_CHECK_LAUNCH("layernorm_fwd");
  return 0;
}

template <typename T>
int ln_bwd_launch(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                  float* dgamma, float* dbeta, void* ws, int64_t rows, int C, hipStream_t s, const void* dres = nullptr, int* nblocks = nullptr) {
  DGTD_REQUIRE(C % Vec16<T>::N == 0, "layernorm: C=%d must be a multiple of %d", C, Vec16<T>::N);
  LnGeom g = ln_geom<T>(C);
  DGTD_REQUIRE(g.npl <= LN_MAX_NPL, "layernorm: C=%d too large", C);
  DGTD_REQUIRE(rows > 0, "layernorm_bwd: rows must be > 0");
  int grid = (int)std::min<int64_t>(cdiv(rows, g.rows_per_block * 4), LN_BWD_MAX_GRID);
  size_t lds = (size_t)4 * 2 * C * sizeof(float);
  LN_DISPATCH(g, hipLaunchKernelGGL((ln_bwd_kernel<T, NPL_, G_>), dim3(grid), dim3(256), lds, s, (const T*)dy, (const T*)x, gamma, mean, rstd, (const T*)dres, (T*)dx, (float*)ws, rows, C));
  DGTD_CHECK_LAUNCH("layernorm_bwd");
  if (nblocks) { *nblocks = grid; return 0; }
  const dgtd_reduce_entry e{(const float*)ws, grid, 2 * C, dgamma, C, dbeta, DGTD_F32, 0, 0, nullptr};     // ws [grid][2C] = { dgamma | dbeta } partial rows
  return dgtd_multi_reduce_impl(&e, 1, s);
}

}  // namespace

extern "C" int dgtd_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                  int64_t rows, int C, float eps, dgtd_dtype dt, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, 2.0 * dgtd_esize(dt) * rows * C, "dgtd_layernorm_fwd[rows=%lld,C=%d]", (long long)rows, C);
  DGTD_REQUIRE(DGTD_IS_HALF(dt) || dt == DGTD_F32, "layernorm_fwd: bad dtype %d", (int)dt);
  DGTD_DISPATCH(dt, return ln_fwd_launch<T_>(x, gamma, beta, y, mean, rstd, rows, C, eps, (hipStream_t)s));
}

extern "C" int dgtd_layernorm_bwd_add(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                                      const void* dx_add, void* dx, float* dgamma, float* dbeta, void* workspace, int64_t rows, int C,
                                      dgtd_dtype dt, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (dx_add ? 4.0 : 3.0) * dgtd_esize(dt) * rows * C, "dgtd_layernorm_bwd[rows=%lld,C=%d]", (long long)rows, C);
  DGTD_REQUIRE(DGTD_IS_HALF(dt) || dt == DGTD_F32, "layernorm_bwd_add: bad dtype %d", (int)dt);
  DGTD_DISPATCH(dt, return ln_bwd_launch<T_>(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, workspace, rows, C, (hipStream_t)s, dx_add));
}

extern "C" int dgtd_layernorm_bwd_partial(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                                          const void* dx_add, void* dx, void* workspace, int64_t rows, int C, dgtd_dtype dt, int* nblocks,
                                          dgtd_stream s) {
  DGTD_REQUIRE(nblocks, "layernorm_bwd_partial: nblocks is NULL");
  DGTD_PROF(s, DGTD_HBM, (dx_add ? 4.0 : 3.0) * dgtd_esize(dt) * rows * C, "dgtd_layernorm_bwd[rows=%lld,C=%d]", (long long)rows, C);
  DGTD_REQUIRE(DGTD_IS_HALF(dt) || dt == DGTD_F32, "layernorm_bwd_partial: bad dtype %d", (int)dt);
  DGTD_DISPATCH(dt, return ln_bwd_launch<T_>(dy, x, gamma, mean, rstd, dx, nullptr, nullptr, workspace, rows, C, (hipStream_t)s, dx_add, nblocks));
}

extern "C" int64_t dgtd_layernorm_bwd_workspace(int C) { return (int64_t)LN_BWD_MAX_GRID * 2 * C * sizeof(float); }

extern "C" int dgtd_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                                  void* dx, float* dgamma, float* dbeta, void* workspace, int64_t rows, int C,
                                  dgtd_dtype dt, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, 3.0 * dgtd_esize(dt) * rows * C, "dgtd_layernorm_bwd[rows=%lld,C=%d]", (long long)rows, C);
  DGTD_REQUIRE(DGTD_IS_HALF(dt) || dt == DGTD_F32, "layernorm_bwd: bad dtype %d", (int)dt);
  DGTD_DISPATCH(dt, return ln_bwd_launch<T_>(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, workspace, rows, C, (hipStream_t)s));
}
