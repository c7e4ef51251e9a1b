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
//   LDS    : (TY + K - 1) x (TXW + K - 1) x 128 bf16/fp32, rounded up to 4 KB  (K = 7: 56 KB bf16)
#include "common.h"

namespace {

constexpr int TY = 4, TXW = 16, TXS = 8;   // TXS = strip of outputs a lane computes at a time

// The 16-byte global loads that bring rows [y0 - P, y0 + TY + P) x cols [x0 - P, x0 + TXW + P) x channels [cb*128, +128) of image b
// to a workgroup, zero padded, and their LDS stores.  load() only issues: a position outside the image (and the slots past the
// tile's end) reads a clamped, always-valid address and its value is dropped by a select in store(), and the LDS tile is rounded
// up to whole 256-thread passes (SLOTS), so neither a load nor a store stands under control flow and no wait separates the loads.  The kernel issues its other global loads between the two calls:
// everything a workgroup needs from memory arrives with one round trip of latency.
template <typename T, int K>
struct TileStage {
  typedef typename Vec16<T>::type VT;
  static constexpr int V = Vec16<T>::N, P = K / 2, RW = TXW + K - 1, RH = TY + K - 1, CPP = 128 / V;   // 16-B chunks per position
  static constexpr int TOTAL = RH * RW * CPP, NCH = (TOTAL + 255) / 256, SLOTS = NCH * 256;
  VT v[NCH];
  bool ok[NCH];
  __device__ __forceinline__ void load(const T* __restrict__ x, int b, int y0, int x0, int cb, int H, int W, int C, int tid) {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int i = tid + k * 256;
      const int ch = i % CPP, pos = i / CPP, xx = pos % RW, yy = pos / RW;
      const int gy = y0 + yy - P, gx = x0 + xx - P;
      ok[k] = i < TOTAL && gy >= 0 && gy < H && gx >= 0 && gx < W;
      const int cy = min(max(gy, 0), H - 1), cx = min(max(gx, 0), W - 1);
      v[k] = *reinterpret_cast<const VT*>(x + (((size_t)b * H + cy) * W + cx) * C + cb * 128 + ch * V);
    }
  }
  __device__ __forceinline__ void store(T* __restrict__ tile, int tid) const {
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int i = tid + k * 256;
      VT o;
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = ok[k] ? v[k][j] : (T)0.f;
      *reinterpret_cast<VT*>(tile + (size_t)i * V) = o;   // pos * 128 + ch * V == i * V; the slots past TOTAL are LDS slack
    }
  }
};

// the value of a 4- or 8-byte register operand is computed (and a load behind it complete) at this point of the program: an empty
// asm the optimiser can neither look through nor move a producer across
template <typename P>
__device__ __forceinline__ void pin_here(P& v) {
  static_assert(sizeof(P) == 4 || sizeof(P) == 8, "pin_here: one or two registers");
  if constexpr (sizeof(P) == 4) { unsigned u = __builtin_bit_cast(unsigned, v); asm volatile("" : "+v"(u)); v = __builtin_bit_cast(P, u); }
  else { unsigned long long u = __builtin_bit_cast(unsigned long long, v); asm volatile("" : "+v"(u)); v = __builtin_bit_cast(P, u); }
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
  TileStage<T, K> st;
  st.load(x, b, y0, x0, cb, H, W, C, tid);
  // all K*K taps of this lane's two channels, and the bias, stay in registers
  // the lane's two channels travel as float2 values: the multiply-adds compile to v_pk_fma_f32 (two FMAs per VALU instruction)
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 w[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) { w[i][0] = wt[(size_t)i * C + c0]; w[i][1] = wt[(size_t)i * C + c0 + 1]; }
  const float* bp = bias ? bias : wt;      // no bias: a valid address, the value is dropped
  const float b0 = bp[c0], b1 = bp[c0 + 1];
  f2 bv;
  bv[0] = bias ? b0 : 0.f; bv[1] = bias ? b1 : 0.f;
  const int oy = y0 + wave;                       // this wave's output row
  // modes 2 and 3: the aux values of the wave's outputs, first and second strip, in the same round trip (outputs past the image's
  // edge read a clamped address: no load under a branch)
  static_assert(TXW == 2 * TXS, "the aux prefetch holds two strips");
  PT ax[TXS], ax_next[TXS];
  if (MODE >= 2) {
    const size_t arow = ((size_t)b * H + min(oy, H - 1)) * W;
#pragma unroll
    for (int i = 0; i < TXS; ++i) {
      ax[i] = *reinterpret_cast<const PT*>(aux + (arow + min(x0 + i, W - 1)) * C + c0);
      ax_next[i] = *reinterpret_cast<const PT*>(aux + (arow + min(x0 + TXS + i, W - 1)) * C + c0);
    }
  }
  __builtin_amdgcn_sched_barrier(0);              // every global load above is issued before the first LDS store waits for one
  st.store(tile, tid);
  __syncthreads();
  // a wave whose row lies past the image's end runs on (its LDS rows exist) and stores nothing: an early exit here would be a
  // block for the compiler to sink the tap loads into, behind the barrier
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
    // the sums are complete HERE.  Without this the compiler sinks each output's 49 multiply-adds into the `ox < W` block of its
    // store: eight dependent chains one after another, with all 7 x 14 staged inputs of the strip held in registers for them.
    // The same holds for an aux load, which would start its round trip only there.
#pragma unroll
    for (int i = 0; i < TXS; ++i) { pin_here(acc[i]); if (MODE >= 2) pin_here(ax[i]); }
#pragma unroll
    for (int i = 0; i < TXS; ++i) {
      const int ox = x0 + sx + i;
      if (ox < W && oy < H) {
        const size_t o = (((size_t)b * H + oy) * W + ox) * C + c0;
        PT r;
        if (MODE == 2) {
          const PT g = ax[i];
          r[0] = (T)((float)g[0] * gelu_grad_fast(acc[i][0])); r[1] = (T)((float)g[1] * gelu_grad_fast(acc[i][1]));
        } else if (MODE == 1) {
          r[0] = (T)gelu_fast(acc[i][0]); r[1] = (T)gelu_fast(acc[i][1]);
        } else if (MODE == 3) {
          const PT g = ax[i];
          r[0] = (T)(acc[i][0] + (float)g[0]); r[1] = (T)(acc[i][1] + (float)g[1]);
        } else {
          r[0] = (T)acc[i][0]; r[1] = (T)acc[i][1];
        }
        *reinterpret_cast<PT*>(y + o) = r;
      }
    }
    if (MODE >= 2) {
#pragma unroll
      for (int i = 0; i < TXS; ++i) ax[i] = ax_next[i];
    }
  }
}

template <typename T, int K> constexpr size_t fwd_lds() { return (size_t)TileStage<T, K>::SLOTS * 16; }

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
