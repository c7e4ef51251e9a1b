// dwconv_tiled.hip — LDS-tiled depthwise 7x7 convolution on NHWC tensors (C % 128 == 0): forward / backward-data (same kernel,
// flipped filter).  Same math as the direct kernel of dwconv.hip, which stays the fallback for other channel counts and whose C ABI
// entry dgtd_dwconv_fwd calls dgtd_dwconv_tiled_fwd below.  The weight gradient has no tiled variant: it lost to the direct
// K-wave kernel on every shape of the model.
//
// Why: with lanes along channels there is no reuse between lanes, and the K-fold row reuse of the direct kernel had to come out
// of L1/L2 — measured (rocprofv3 PMC) it was bounded by the L1 path and by waiting, at 5-10 % of the HBM roofline although its
// HBM traffic was already minimal.  Here a workgroup stages the input tile WITH its halo into LDS once (coalesced 16-B copies),
// every lane keeps all K*K taps of its 2 channels in registers, and the inner loop is LDS reads + FMAs only.
//   tile   : TY = 4 output rows (one per wave) x TXW = 16 output columns x 128 channels (64 lanes x 2)
//   LDS    : (TY + K - 1) x (TXW + K - 1) x 128 bf16/fp32  (K = 7: 56 KB bf16)
#include "common.h"

namespace {

constexpr int TY = 4, TXW = 16, TXS = 8;   // TXS = strip of outputs a lane computes at a time

// stage rows [y0 - P, y0 + TY + P) x cols [x0 - P, x0 + TXW + P) x channels [cb*128, +128) of image b into LDS, zero padded.
// All of a thread's 16-byte loads are issued before the first LDS store (fully unrolled, registers), so the tile arrives with
// one round trip of latency instead of one per chunk.
template <typename T, int K>
__device__ __forceinline__ void stage_tile(T* __restrict__ tile, const T* __restrict__ x, int b, int y0, int x0, int cb, int H, int W,
                                           int C, int tid) {
  typedef typename Vec16<T>::type VT;
  constexpr int V = Vec16<T>::N, P = K / 2, RW = TXW + K - 1, RH = TY + K - 1, CPP = 128 / V;   // 16-B chunks per position
  constexpr int TOTAL = RH * RW * CPP, NCH = (TOTAL + 255) / 256;
  VT v[NCH];
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int i = tid + k * 256;
    const int ch = i % CPP, pos = i / CPP, xx = pos % RW, yy = pos / RW;
    const int gy = y0 + yy - P, gx = x0 + xx - P;
    if (i < TOTAL && gy >= 0 && gy < H && gx >= 0 && gx < W) v[k] = *reinterpret_cast<const VT*>(x + (((size_t)b * H + gy) * W + gx) * C + cb * 128 + ch * V);
    else
#pragma unroll
      for (int j = 0; j < V; ++j) v[k][j] = (T)0.f;
  }
#pragma unroll
  for (int k = 0; k < NCH; ++k) {
    const int i = tid + k * 256;
    if (i < TOTAL) *reinterpret_cast<VT*>(tile + (size_t)i * V) = v[k];   // pos * 128 + ch * V == i * V
  }
}

// MODE 0: y = conv + bias   MODE 1: y = gelu(conv + bias)   MODE 2: y = aux * gelu'(conv + bias)   MODE 3: y = conv + bias + aux
template <typename T, int K, int MODE>
__global__ __launch_bounds__(256) void dwconv_tiled_fwd_kernel(const T* __restrict__ x, const float* __restrict__ wt,
                                                               const float* __restrict__ bias, const T* __restrict__ aux,
                                                               T* __restrict__ y, int B, int H, int W, int C) {
  typedef typename Vec2<T>::type PT;
  constexpr int P = K / 2, RW = TXW + K - 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* tile = reinterpret_cast<T*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ncb = C / 128, txn = (W + TXW - 1) / TXW, tyn = (H + TY - 1) / TY;
  // XCD-aware remap (guide T1): logically adjacent tiles (next rows of the same column band) share an XCD's L2
  const int nb = gridDim.x, xcd = blockIdx.x & 7, qn = nb >> 3, rn = nb & 7;
  int t = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + (blockIdx.x >> 3);
  const int cb = t % ncb; t /= ncb;
  const int ty = t % tyn; t /= tyn;
  const int tx = t % txn;
  const int b = t / txn;
  const int y0 = ty * TY, x0 = tx * TXW, c0 = cb * 128 + lane * 2;
  stage_tile<T, K>(tile, x, b, y0, x0, cb, H, W, C, tid);
  // all K*K taps of this lane's two channels, and the bias, stay in registers (loaded behind the tile: the staging registers are dead)
  // the lane's two channels travel as float2 values: the multiply-adds compile to v_pk_fma_f32 (two FMAs per VALU instruction)
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 w[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) { w[i][0] = wt[(size_t)i * C + c0]; w[i][1] = wt[(size_t)i * C + c0 + 1]; }
  f2 bv;
  bv[0] = bias ? bias[c0] : 0.f; bv[1] = bias ? bias[c0 + 1] : 0.f;
  __syncthreads();
  const int oy = y0 + wave;                       // this wave's output row
  if (oy >= H) return;
#pragma unroll 1
  for (int s = 0; s < TXW / TXS; ++s) {
    const int sx = s * TXS;
    if (x0 + sx >= W) break;
    f2 acc[TXS];
#pragma unroll
    for (int i = 0; i < TXS; ++i) acc[i] = bv;
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      f2 in[TXS + K - 1];
      const T* row = tile + ((size_t)(wave + ky) * RW + sx) * 128 + lane * 2;
#pragma unroll
      for (int i = 0; i < TXS + K - 1; ++i) {
        PT v = *reinterpret_cast<const PT*>(row + (size_t)i * 128);
        in[i][0] = (float)v[0]; in[i][1] = (float)v[1];
      }
#pragma unroll
      for (int kx = 0; kx < K; ++kx)
#pragma unroll
        for (int i = 0; i < TXS; ++i) acc[i] = __builtin_elementwise_fma(in[i + kx], w[ky * K + kx], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < TXS; ++i) {
      const int ox = x0 + sx + i;
      if (ox < W) {
        const size_t o = (((size_t)b * H + oy) * W + ox) * C + c0;
        PT r;
        if (MODE == 2) {
          PT g = *reinterpret_cast<const PT*>(aux + o);
          r[0] = (T)((float)g[0] * gelu_grad_fast(acc[i][0])); r[1] = (T)((float)g[1] * gelu_grad_fast(acc[i][1]));
        } else if (MODE == 1) {
          r[0] = (T)gelu_fast(acc[i][0]); r[1] = (T)gelu_fast(acc[i][1]);
        } else if (MODE == 3) {
          PT g = *reinterpret_cast<const PT*>(aux + o);
          r[0] = (T)(acc[i][0] + (float)g[0]); r[1] = (T)(acc[i][1] + (float)g[1]);
        } else {
          r[0] = (T)acc[i][0]; r[1] = (T)acc[i][1];
        }
        *reinterpret_cast<PT*>(y + o) = r;
      }
    }
  }
}

template <typename T, int K> constexpr size_t fwd_lds() { return (size_t)(TY + K - 1) * (TXW + K - 1) * 128 * sizeof(T); }

}  // namespace

// ---- entry point used by dwconv.hip's dgtd_dwconv_fwd when K == 7 and C % 128 == 0 ----------------------------------------------
template <typename T, int K>
static int tiled_fwd(const void* x, const float* wt, const float* bias, const void* aux, void* y, int B, int H, int W, int C, int mode,
                     hipStream_t s) {
  const int64_t tiles = (int64_t)B * cdiv(H, TY) * cdiv(W, TXW) * (C / 128);
  DGTD_REQUIRE(tiles < (1LL << 31), "dwconv_tiled_fwd: too many tiles");
  const size_t lds = fwd_lds<T, K>();
#define TILED(MODE) hipLaunchKernelGGL((dwconv_tiled_fwd_kernel<T, K, MODE>), dim3((unsigned)tiles), dim3(256), lds, s, (const T*)x, wt, bias, (const T*)aux, (T*)y, B, H, W, C)
  if (mode == 0) TILED(0); else if (mode == 1) TILED(1); else if (mode == 2) TILED(2); else TILED(3);
#undef TILED
  DGTD_CHECK_LAUNCH("dwconv_tiled_fwd");
  return 0;
}

int dgtd_dwconv_tiled_fwd(const void* x, const float* wt, const float* bias, const void* aux, void* y, int B, int H, int W, int C, int K,
                          int mode, dgtd_dtype dt, hipStream_t s) {
  DGTD_REQUIRE(K == 7, "dwconv_tiled_fwd: K=%d (the tiled kernel serves 7x7 only)", K);
  DGTD_DISPATCH(dt, return (tiled_fwd<T_, 7>(x, wt, bias, aux, y, B, H, W, C, mode, s)));
}
