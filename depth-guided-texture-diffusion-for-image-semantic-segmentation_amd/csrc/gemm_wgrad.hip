// gemm_wgrad.hip — the weight gradients of the Linear layers as a hand-written MFMA GEMM that reduces over TOKENS (gfx950, wave = 64).
//
//   dW[z][N,K] = sum_m dY[z][m,N] · X[z][m,K]      z < batch, per-batch element strides s_dy / s_x / s_dw
//
// (pwconv1/2 of the ConvNeXt stages, q / kv / proj / fc1 / fc2 of the PVT blocks: the strided-batched runs of the deferred phase and the
// per-layer path of csrc_torch/bindings.cpp.)  Both operands are contiguous along the dimension that is NOT reduced, the opposite of
// gemm.hip: no transposed copy of dY or X is ever made in global memory, the transpose happens in the LDS read.
//
// Workgroup = one TN x TK output tile (TN, TK = 128 or 64 each: N = 320, 1280 and 64 are no multiples of 128) of one batch entry x one
// chunk of the token dimension; 4 waves as 2 (n) x 2 (k), wave tile TN/2 x TK/2 of v_mfma_f32_32x32x16_{bf16,f16}, fp32 accumulators.
// k-step = 64 tokens.  LDS image of a stage: the dY tile [64 tokens][TN] followed by the X tile [64 tokens][TK], token-major exactly as
// in global memory, filled with 16-byte LDS-DMA (global_load_lds_dwordx4, lane-linear 1-KiB pieces = 4 rows of 256 B or 8 rows of 128 B),
// two stages, the next step's tiles in flight across the barrier (counted vmcnt, raw s_barrier) - gemm.hip's two-stage form.  Both MFMA
// operands are taken with the transposing read (ds_read_b64_tr_b16, two per fragment): per 32-lane half one read covers 4 token rows x
// 64 bytes, which on plain 256-byte rows would put all 4 rows on the same 16 banks (4-way), on 128-byte rows 2-way.  The 64-byte group
// index of a row is therefore XOR-ed with (token & 3) [256-byte rows] or ((token >> 1) & 1) [128-byte rows] ON THE GLOBAL SOURCE ADDRESS
// of the DMA (the LDS side of the DMA stays lane-linear); the four rows of a read then sit on four disjoint 16-bank ranges.  The XOR
// moves whole 64-byte groups, so the 4 x 16-element blocks of the transposing read stay contiguous.  Both fragments of a 16-token slice
// carry the same token permutation (element j of lane half h = token 8 (j >> 2) + 4 h + (j & 3)), so the products pair up.
// MFMA orientation: first operand = X fragment, second = dY fragment, so lane & 31 = output row n of its 32-row block and registers
// 4 q .. 4 q + 3 = output columns k = 8 q + 4 h + {0..3}.  The accumulators go through LDS once (the stages are dead by then) and every
// global store is a coalesced row-major 16- or 32-byte store.
//
// Token chunks: the host picks S so that batch x tiles x S fills the chip; every workgroup writes a PLAIN fp32 partial tile into the
// caller's workspace [batch][S][N·K] (no atomics, nothing to zero), and a second kernel sums the S partials in a fixed order and rounds
// ONCE to the 16-bit gradient.  S == 1: the kernel rounds and stores dW itself.  Bit-reproducible from launch to launch either way.
//
// Bound: per token step a workgroup reads 64 (TN + TK) e bytes for 2·64·TN·TK flop = TN TK / (TN + TK) flop/B = 64 flop/B at 128 x 128
// from L2 / MALL, but from HBM every operand byte is needed once per launch if the tiles of a chunk run together: 2 M N K flop over
// e (M N + M K) + partial traffic, i.e. 2 N K / (e (N + K)) flop/B: 102 flop/B at (N, K) = (512, 128), 410 at (2048, 512), 819 at
// (4096, 1024) against the 312 flop/B ridge - HBM-bound at ConvNeXt stages 0-1 and the PVT shapes, MFMA-bound at stages 2-3.
#include "common.h"
#include <algorithm>

namespace {

constexpr int TS = 64;                                     // tokens per k-step
constexpr int MAX_CHUNK_STEPS = 64;                        // a chunk is at most 4096 tokens

struct WgradArgs {
  const void* dy;         // [batch] x [M,N]
  const void* x;          // [batch] x [M,K]
  void* dw;               // [batch] x [N,K] in T (written when S == 1)
  float* ws;              // [batch][S][N·K] fp32 partials (written when S > 1)
  int M, N, K, tiles_k;
  int S, per;             // token chunks, k-steps per chunk (the last chunk may be shorter)
  int64_t s_dy, s_x, s_dw;
};

typedef __attribute__((address_space(3))) void* lds_void_ptr;
typedef const __attribute__((address_space(1))) void* glb_void_ptr;

// one 16-byte LDS-DMA per lane: LDS destination = wave-uniform base + lane * 16
__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((glb_void_ptr)gsrc, (lds_void_ptr)lds_wave_base, 16, 0, 0);
}
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// lds_tr_frag (common.h) on the swizzled image: W = row length in elements (128 or 64), grp = 32-column group of the fragment.
// Every lane's row has (row & 3) = (lane & 15) >> 2 in both reads (row0 is a multiple of 16), so the swizzle is a per-lane constant.
template <typename T, int W>
__device__ __forceinline__ typename Vec16<T>::type tr_frag_sw(const T* tile, int row0, int grp, int lane) {
  const int i = lane & 15, g1 = (lane >> 4) & 1, h = lane >> 5;
  const int sw = W == 128 ? (i >> 2) : ((i >> 3) & 1);
  const T* p = tile + (row0 + 4 * h + (i >> 2)) * W + ((grp ^ sw) << 5) + 16 * g1 + 4 * (i & 3);
  typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
  typedef typename Vec8<T>::type V4;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 8 * W));
  V4 l4 = __builtin_bit_cast(V4, lo), h4 = __builtin_bit_cast(V4, hi);
  typename Vec16<T>::type f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[j] = l4[j]; f[4 + j] = h4[j]; }
  return f;
}

template <typename T, int TN, int TK>
__global__ __launch_bounds__(256, 2) void gemm_wgrad_kernel(const WgradArgs g) {
  typedef typename Vec16<T>::type V8;
  constexpr int WN = TN / 2, WK = TK / 2, NI = WN / 32, KI = WK / 32;   // wave tile and its 32x32 MFMA tiles
  constexpr int DY_BYTES = TS * TN * 2, X_BYTES = TS * TK * 2, STAGE = DY_BYTES + X_BYTES;
  constexpr int SROW = TK * 4 + 16;                        // fp32 staging row stride in bytes (+16: conflict-free 16-byte column writes)
  constexpr int LDS_BYTES = 2 * STAGE > TN * SROW ? 2 * STAGE : TN * SROW;
  constexpr int DY_PER_WAVE = (TN / 8) / 4, X_PER_WAVE = (TK / 8) / 4;  // 1-KiB DMA pieces per wave and stage
  constexpr int DY_CPR = TN / 8, X_CPR = TK / 8;            // 16-byte chunks per tile row
  constexpr int PIECES = DY_PER_WAVE + X_PER_WAVE;
  __shared__ __attribute__((aligned(1024))) char lds[LDS_BYTES];        // the ONLY LDS object

  const int tile = blockIdx.x, chunk = blockIdx.y, z = blockIdx.z;
  const int tn = tile / g.tiles_k, tk = tile - tn * g.tiles_k;
  const int n0 = tn * TN, k0 = tk * TK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = g.N, K = g.K;
  const int step0 = chunk * g.per;
  const int steps = g.M / TS;
  const int nk = steps - step0 < g.per ? steps - step0 : g.per;         // >= 1: the host never makes an empty chunk

  const T* DYg = (const T*)g.dy + (size_t)z * g.s_dy + (size_t)step0 * TS * N + n0;
  const T* Xg = (const T*)g.x + (size_t)z * g.s_x + (size_t)step0 * TS * K + k0;
  // per-lane source offsets of the DMA pieces (elements, without the token offset): the 64-byte group of the source chunk is swizzled
  int dy_off[DY_PER_WAVE], x_off[X_PER_WAVE];
#pragma unroll
  for (int p = 0; p < DY_PER_WAVE; ++p) {
    const int row = (wave * DY_PER_WAVE + p) * (64 / DY_CPR) + lane / DY_CPR, c = lane % DY_CPR;
    const int sw = TN == 128 ? (row & 3) << 2 : ((row >> 1) & 1) << 2;
    dy_off[p] = row * N + ((c ^ sw) << 3);
  }
#pragma unroll
  for (int p = 0; p < X_PER_WAVE; ++p) {
    const int row = (wave * X_PER_WAVE + p) * (64 / X_CPR) + lane / X_CPR, c = lane % X_CPR;
    const int sw = TK == 128 ? (row & 3) << 2 : ((row >> 1) & 1) << 2;
    x_off[p] = row * K + ((c ^ sw) << 3);
  }
  // this wave's share of token step kt -> stage st; the token offset rides on the UNIFORM base pointer
  auto stage = [&](int kt, int st) {
    char* sa = lds + st * STAGE;
    char* sb = sa + DY_BYTES;
    const T* dyk = DYg + (size_t)kt * TS * N;
    const T* xk = Xg + (size_t)kt * TS * K;
#pragma unroll
    for (int p = 0; p < DY_PER_WAVE; ++p) glds16(dyk + dy_off[p], sa + (wave * DY_PER_WAVE + p) * 1024);
#pragma unroll
    for (int p = 0; p < X_PER_WAVE; ++p) glds16(xk + x_off[p], sb + (wave * X_PER_WAVE + p) * 1024);
  };

  const int wn = wave >> 1, wk = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  f32x16 acc[NI][KI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int ki = 0; ki < KI; ++ki)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[ni][ki][e] = 0.f;

  // one 16-token slice: fragments double-buffered in registers (the reads of slice kk + 1 fly while the MFMAs of slice kk issue)
  V8 dyf[2][NI], xf[2][KI];
  auto frags = [&](const char* sa, const char* sb, int kk, int set) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) dyf[set][ni] = tr_frag_sw<T, TN>((const T*)sa, 16 * kk, (wn * WN) / 32 + ni, lane);
#pragma unroll
    for (int ki = 0; ki < KI; ++ki) xf[set][ki] = tr_frag_sw<T, TK>((const T*)sb, 16 * kk, (wk * WK) / 32 + ki, lane);
  };
  auto mfmas = [&](int set) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int ki = 0; ki < KI; ++ki) acc[ni][ki] = mfma16(xf[set][ki], dyf[set][ni], acc[ni][ki]);   // lane & 31 = output ROW n
    __builtin_amdgcn_s_setprio(0);
  };
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nk) {
      stage(kt + 1, st ^ 1);                               // its buffer was last read before the closing barrier of step kt - 1
      wait_vmcnt<PIECES>();                                // all but the pieces just issued: step kt has landed (this wave's share)
    } else {
      wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();                          // ... and everybody else's share
    const char* sa = lds + st * STAGE;
    const char* sb = sa + DY_BYTES;
    frags(sa, sb, 0, 0);
#pragma unroll
    for (int kk = 0; kk < TS / 16; ++kk) {
      if (kk + 1 < TS / 16) frags(sa, sb, kk + 1, (kk + 1) & 1);
      mfmas(kk & 1);
    }
    __builtin_amdgcn_s_barrier();                          // every wave is done reading stage st before step kt + 1 refills it
  }

  // ---- accumulators -> fp32 staging tile [TN][TK] in LDS (the operand stages are dead after the closing barrier)
  // lane (r, h) holds, for output row n = r of its 32-row block, columns 8 q + 4 h + {0..3} (registers 4q .. 4q+3)
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int ki = 0; ki < KI; ++ki) {
      char* base = lds + (wn * WN + ni * 32 + r) * SROW + (wk * WK + ki * 32 + 4 * h) * 4;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[ni][ki][4 * qd + e];
        *reinterpret_cast<f32x4*>(base + qd * 32) = v;
      }
    }
  __syncthreads();

  // ---- row-major epilogue: thread = one 8-column chunk, rows tid / CPR + i * RPP
  constexpr int CPR = TK / 8, RPP = 256 / CPR, NPASS = TN / RPP;
  const int cc = tid % CPR, r0 = tid / CPR;
  const bool direct = g.S == 1;
  float* wsp = direct ? nullptr : g.ws + ((size_t)z * g.S + chunk) * ((size_t)N * K);
  T* dwp = (T*)g.dw + (size_t)z * g.s_dw;
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    const int row = r0 + i * RPP;
    const char* sp = lds + row * SROW + cc * 32;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(sp), hi = *reinterpret_cast<const f32x4*>(sp + 16);
    const size_t o = (size_t)(n0 + row) * K + k0 + cc * 8;
    if (direct) {
      V8 out;
#pragma unroll
      for (int e = 0; e < 4; ++e) { out[e] = (T)lo[e]; out[4 + e] = (T)hi[e]; }
      *reinterpret_cast<V8*>(dwp + o) = out;
    } else {
      *reinterpret_cast<f32x4*>(wsp + o) = lo;
      *reinterpret_cast<f32x4*>(wsp + o + 4) = hi;
    }
  }
}

// Second stage: dW[z][c] = round(ws[z][0][c] + ws[z][1][c] + ... + ws[z][S-1][c]), fp32, fixed order, one rounding.  A kernel of its own
// instead of a dgtd_multi_reduce entry per batch item: that kernel gives one workgroup 32 columns x 8 row groups with 4-byte loads and
// 2-byte stores, sized for the small latency-bound partial buffers of the column reductions ([a few hundred rows][<= a few thousand
// columns]).  Here the shape is the opposite, S = 2 .. 8 rows of N·K = 64K .. 4M columns: an entry would need N·K / 32 workgroups (131072
// per layer at N·K = 4M, 27 layers per stage) that read 128 bytes per row each with at most S of their 8 row groups busy.  This one
// streams: a thread owns 8 adjacent columns, reads S x 32 bytes and writes 16.
template <typename T>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* ws, void* dw, int S, int64_t nk, int64_t s_dw) {
  typedef typename Vec16<T>::type V8;
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
  if (c >= nk) return;
  const int z = blockIdx.y;
  const float* p = ws + (size_t)z * S * nk + c;
  f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
  for (int s = 1; s < S; ++s) {
    const float* q = p + (size_t)s * nk;
    lo += *reinterpret_cast<const f32x4*>(q);
    hi += *reinterpret_cast<const f32x4*>(q + 4);
  }
  V8 out;
#pragma unroll
  for (int e = 0; e < 4; ++e) { out[e] = (T)lo[e]; out[4 + e] = (T)hi[e]; }
  *reinterpret_cast<V8*>((T*)dw + (size_t)z * s_dw + c) = out;
}

inline int tile_n(int N) { return N % 128 == 0 ? 128 : 64; }

// k-steps per token chunk.  The split aims at two workgroups per CU (256 CUs) from batch x tiles x S.  A chunk is never longer than
// MAX_CHUNK_STEPS x 64 = 4096 tokens: the bound of the numerics tests, C_MFMA = 2^-21 relative to sum |dy||x|, is stated for fp32 MFMA
// accumulation chains of that length (tests/_numerics.py), and a longer chain would void it.  It is not shorter than 8 steps (512
// tokens) unless M is: a workgroup's partial tile (TN·TK·4 bytes) then stays below a quarter of the operand bytes it reads.
inline int chunk_steps(int batch, int M, int N, int K) {
  const int steps = M / TS;
  const int64_t wgs = (int64_t)batch * (N / tile_n(N)) * (K / tile_n(K));
  const int want = (int)std::max<int64_t>(1, cdiv(512, wgs));
  int per = std::max(steps / want, std::min(steps, 8));
  return std::min(per, MAX_CHUNK_STEPS);
}

template <typename T>
int launch(const WgradArgs& a, int batch, hipStream_t st) {
  const int TN = tile_n(a.N), TK = tile_n(a.K);
  const dim3 grid((a.N / TN) * (a.K / TK), a.S, batch), block(256);
  if (TN == 128 && TK == 128) hipLaunchKernelGGL((gemm_wgrad_kernel<T, 128, 128>), grid, block, 0, st, a);
  else if (TN == 128) hipLaunchKernelGGL((gemm_wgrad_kernel<T, 128, 64>), grid, block, 0, st, a);
  else if (TK == 128) hipLaunchKernelGGL((gemm_wgrad_kernel<T, 64, 128>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((gemm_wgrad_kernel<T, 64, 64>), grid, block, 0, st, a);
  DGTD_CHECK_LAUNCH("gemm_wgrad");
  if (a.S > 1) {
    const int64_t nk = (int64_t)a.N * a.K;
    hipLaunchKernelGGL((wgrad_reduce_kernel<T>), dim3((unsigned)cdiv(nk / 8, 256), batch), dim3(256), 0, st, a.ws, a.dw, a.S, nk, a.s_dw);
    DGTD_CHECK_LAUNCH("gemm_wgrad_reduce");
  }
  return 0;
}

}  // namespace

extern "C" int dgtd_gemm_wgrad_supported(int M, int N, int K, dgtd_dtype dt) {
  return DGTD_IS_HALF(dt) && M > 0 && N > 0 && K > 0 && M % TS == 0 && N % 64 == 0 && K % 64 == 0 && (int64_t)M * N < (1ll << 31) &&
         (int64_t)M * K < (1ll << 31) && (int64_t)N * K < (1ll << 31) ? 1 : 0;
}

extern "C" int64_t dgtd_gemm_wgrad_workspace(int batch, int M, int N, int K) {
  if (batch <= 0 || !dgtd_gemm_wgrad_supported(M, N, K, DGTD_BF16)) return 0;
  const int S = (int)cdiv(M / TS, chunk_steps(batch, M, N, K));
  return (int64_t)batch * S * N * K * 4;
}

extern "C" int dgtd_gemm_wgrad_batched(const void* dy, const void* x, void* dw, void* workspace, int batch, int M, int N, int K, int64_t s_dy,
                                       int64_t s_x, int64_t s_dw, dgtd_dtype dt, dgtd_stream s) {
  const double prof_flops = 2.0 * batch * M * N * K, prof_bytes = (double)dgtd_esize(dt) * batch * ((double)M * N + (double)M * K + (double)N * K);
  const bool prof_mfma = prof_flops > 312.5 * prof_bytes;
  DGTD_PROF(s, prof_mfma ? DGTD_MFMA : DGTD_HBM, prof_mfma ? prof_flops : prof_bytes, "dgtd_gemm_wgrad[b=%d,M=%d,N=%d,K=%d]", batch, M, N, K);
  DGTD_REQUIRE(dy && x && dw, "gemm_wgrad: null operand");
  DGTD_REQUIRE(DGTD_IS_HALF(dt), "gemm_wgrad: bf16 / fp16 only (dtype %d)", (int)dt);
  DGTD_REQUIRE(batch > 0 && batch <= 65535, "gemm_wgrad: batch=%d out of range", batch);
  DGTD_REQUIRE(dgtd_gemm_wgrad_supported(M, N, K, dt), "gemm_wgrad: unsupported shape M=%d N=%d K=%d (M %% 64, N %% 64, K %% 64 must be 0)", M, N, K);
  DGTD_REQUIRE(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw) % 16 == 0, "gemm_wgrad: operands must be 16-byte aligned");
  if (batch > 1) {
    DGTD_REQUIRE(s_dy >= (int64_t)M * N && s_x >= (int64_t)M * K && s_dw >= (int64_t)N * K, "gemm_wgrad: batch strides (%lld, %lld, %lld) overlap the entries",
                 (long long)s_dy, (long long)s_x, (long long)s_dw);
    DGTD_REQUIRE((s_dy | s_x | s_dw) % 8 == 0, "gemm_wgrad: batch strides must keep every entry 16-byte aligned");
  }
  const int per = chunk_steps(batch, M, N, K);
  const int S = (int)cdiv(M / TS, per);
  DGTD_REQUIRE(S == 1 || (workspace && (uintptr_t)workspace % 16 == 0), "gemm_wgrad: %d token chunks need a 16-byte aligned workspace", S);
  WgradArgs a{dy, x, dw, (float*)workspace, M, N, K, K / tile_n(K), S, per, s_dy, s_x, s_dw};
  DGTD_DISPATCH_HALF(dt, return launch<T_>(a, batch, (hipStream_t)s));
}
