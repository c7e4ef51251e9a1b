// common.h — shared device/host helpers for libdgtd.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/dgtd.h"

typedef __bf16 bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- error plumbing (thread-local message, int status) ------------------------------------------
void dgtd_set_error(const char* fmt, ...);
#define DGTD_FAIL(code, ...) do { dgtd_set_error(__VA_ARGS__); return (code); } while (0)
#define DGTD_REQUIRE(cond, ...) do { if (!(cond)) DGTD_FAIL(2, __VA_ARGS__); } while (0)
#define DGTD_CHECK_LAUNCH(name) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) DGTD_FAIL(3, "%s: launch failed: %s", name, hipGetErrorString(e_)); } while (0)

// ---- opt-in per-call device timing (bench.py's roofline leg; off by default: one relaxed atomic load per entry point) -------------
// DGTD_PROF(stream, bound, amount, "key[%d]", ...) at the top of an extern "C" entry point: when dgtd_profile_enable(1) is on, a HIP
// event pair on `stream` brackets everything the entry enqueues; `amount` = algorithmic HBM bytes (bound 0) or MFMA flops (bound 1)
// of the call.  Records are read back with dgtd_profile_dump().  Same key for both host binding layers.
struct DgtdProfScope {
  bool on;
  hipEvent_t a, b;
  hipStream_t st;
  int bound;
  double amount;
  char key[112];
  DgtdProfScope(hipStream_t st, int bound, double amount, const char* fmt, ...) __attribute__((format(printf, 5, 6)));
  ~DgtdProfScope();
};
#define DGTD_PROF(st, bound, amount, ...) DgtdProfScope dgtd_prof_scope_((hipStream_t)(st), (bound), (double)(amount), __VA_ARGS__)
enum { DGTD_HBM = 0, DGTD_MFMA = 1 };
static inline int dgtd_esize(dgtd_dtype dt) { return (dt == DGTD_BF16 || dt == DGTD_F16) ? 2 : (dt == DGTD_F64 ? 8 : 4); }

// ---- scalar load/store as float for both I/O dtypes ---------------------------------------------
template <typename T> __device__ __forceinline__ float to_f(T v) { return (float)v; }
template <typename T> __device__ __forceinline__ T from_f(float v) { return (T)v; }

// 16-byte vector of T: 4 floats or 8 bf16
template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int N = 4; typedef f32x4 type; };
template <> struct Vec16<bf16_t> { static constexpr int N = 8; typedef bf16x8 type; };
template <> struct Vec16<f16_t> { static constexpr int N = 8; typedef f16x8 type; };
// 8-byte vector of a 2-byte type
template <typename T> struct Vec8;
template <> struct Vec8<bf16_t> { typedef bf16x4 type; };
template <> struct Vec8<f16_t> { typedef f16x4 type; };
// two adjacent elements of T (one 4-byte load of a 16-bit type, 8 bytes of fp32): a lane's channel pair in the depthwise kernels
template <typename T> struct Vec2;
template <> struct Vec2<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct Vec2<bf16_t> { typedef bf16_t type __attribute__((ext_vector_type(2))); };
template <> struct Vec2<f16_t> { typedef f16_t type __attribute__((ext_vector_type(2))); };

// the 16-bit MFMA of the I/O type: v_mfma_f32_32x32x16_bf16 / v_mfma_f32_32x32x16_f16 (same shape, same cycles)
__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// the two 16-bit I/O types (DGTD_BF16 / DGTD_F16)
#define DGTD_IS_HALF(dt) ((dt) == DGTD_BF16 || (dt) == DGTD_F16)
// run STMT with T_ bound to the element type of dtype code `dt` (float unless one of the 16-bit codes)
#define DGTD_DISPATCH(dt, STMT) do { if ((dt) == DGTD_BF16) { typedef bf16_t T_; STMT; } else if ((dt) == DGTD_F16) { typedef f16_t T_; STMT; } \
                                     else { typedef float T_; STMT; } } while (0)
// same for the 16-bit types only (callers have checked DGTD_IS_HALF)
#define DGTD_DISPATCH_HALF(dt, STMT) do { if ((dt) == DGTD_F16) { typedef f16_t T_; STMT; } else { typedef bf16_t T_; STMT; } } while (0)
// run STMT with K_ bound to the depthwise filter size (callers have checked K == 3 || K == 7)
#define DGTD_DISPATCH_K37(K, STMT) do { if ((K) == 7) { constexpr int K_ = 7; STMT; } else { constexpr int K_ = 3; STMT; } } while (0)

// launch-geometry knobs (the tools/*_sweep.sh scripts drive them): read once, into a function-local `static const`
static inline long env_int(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }

// ---- lane reductions in registers ------------------------------------------------------------------------------------------------
// Butterfly over lane ^ O with O a compile-time power of two.  Every step is a VALU instruction (DPP or a permlane swap), none is
// an LDS round trip (__shfl_xor compiles to ds_bpermute_b32 + s_waitcnt lgkmcnt(0)):
//   O = 1, 2  : DPP quad_perm [1,0,3,2] / [2,3,0,1]
//   O = 4     : two bank-masked DPP row shifts (lanes 0-3, 8-11 of a row read lane + 4, lanes 4-7, 12-15 read lane - 4)
//   O = 8     : DPP row_ror:8 (a rotation by half a 16-lane row is the exchange itself)
//   O = 16, 32: v_permlane16_swap / v_permlane32_swap of a register with itself.  The swap exchanges the odd rows (upper half) of
//               its first operand with the even rows (lower half) of its second, so of the two results one is the lane's own value
//               and the other its partner's: which is which depends on the lane, and the commutative combine does not care.
struct LaneAdd { __device__ __forceinline__ float operator()(float a, float b) const { return a + b; } };
struct LaneMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

template <int CTRL, int BANK_MASK>
__device__ __forceinline__ float dpp_move(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, 0xF, BANK_MASK, false));
}
// op(v, v of lane ^ O).  INV8 (O = 4 only): the caller guarantees v is the same in lanes l and l ^ 8, see group_reduce.
template <int O, bool INV8 = false, typename Op>
__device__ __forceinline__ float lane_xor_combine(float v, Op op) {
  static_assert(O == 1 || O == 2 || O == 4 || O == 8 || O == 16 || O == 32, "lane_xor_combine: O must be a power of two below 64");
  if constexpr (O == 1) return op(v, dpp_move<0xB1, 0xF>(v, v));
  else if constexpr (O == 2) return op(v, dpp_move<0x4E, 0xF>(v, v));
  else if constexpr (O == 4 && INV8) return op(v, dpp_move<0x124, 0xF>(v, v));                    // row_ror:4
  else if constexpr (O == 4) return op(v, dpp_move<0x114, 0xA>(dpp_move<0x104, 0x5>(v, v), v));   // row_shl:4 | row_shr:4
  else if constexpr (O == 8) return op(v, dpp_move<0x128, 0xF>(v, v));                            // row_ror:8
  else {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto r = (O == 16) ? __builtin_amdgcn_permlane16_swap(u, u, false, false) : __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return op(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
  }
}
// N independent reductions across power-of-two groups of G adjacent lanes, step by step over all of them (N chains in flight
// instead of one).  The tree is the one of a `for (o = G/2; o > 0; o >>= 1) v += shfl_xor(v, o)` loop: lane l pairs with l ^ o,
// o from G/2 DOWN to 1, so a sum has the bits it had with shuffles.  The order matters for more than the bits: row_ror:4 hands lane
// l the value of lane l - 4 (mod 16), which is lane l ^ 4 or lane (l ^ 4) ^ 8; it stands for the xor-4 exchange only because the
// xor-8 step before it has made the values equal in lanes l and l ^ 8.  Do not reorder the steps; G = 8 has no such step before its
// xor-4 and takes the exact form.
template <int G, int N, typename Op>
__device__ __forceinline__ void group_reduce(float (&v)[N], Op op) {
  static_assert(G == 1 || G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "group_reduce: G must be a power of two <= 64");
#pragma unroll
  for (int n = 0; n < N; ++n) if constexpr (G >= 64) v[n] = lane_xor_combine<32>(v[n], op);
#pragma unroll
  for (int n = 0; n < N; ++n) if constexpr (G >= 32) v[n] = lane_xor_combine<16>(v[n], op);
#pragma unroll
  for (int n = 0; n < N; ++n) if constexpr (G >= 16) v[n] = lane_xor_combine<8>(v[n], op);
#pragma unroll
  for (int n = 0; n < N; ++n) if constexpr (G >= 8) v[n] = lane_xor_combine<4, (G >= 16)>(v[n], op);
#pragma unroll
  for (int n = 0; n < N; ++n) if constexpr (G >= 4) v[n] = lane_xor_combine<2>(v[n], op);
#pragma unroll
  for (int n = 0; n < N; ++n) if constexpr (G >= 2) v[n] = lane_xor_combine<1>(v[n], op);
}
// v[n] += v[n] of lane ^ O for all n: one exact exchange step, for trees that do not run from G/2 down
template <int O, int N> __device__ __forceinline__ void lane_xor_add(float (&v)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = lane_xor_combine<O>(v[n], LaneAdd());
}
template <int G, int N> __device__ __forceinline__ void group_sum(float (&v)[N]) { group_reduce<G>(v, LaneAdd()); }
// reduce across a power-of-two sub-group of G adjacent lanes; every lane of the group gets the result
template <int G> __device__ __forceinline__ float group_sum(float v) { float a[1] = {v}; group_reduce<G>(a, LaneAdd()); return a[0]; }
__device__ __forceinline__ float wave_sum(float v) { return group_sum<64>(v); }
__device__ __forceinline__ float wave_max(float v) { float a[1] = {v}; group_reduce<64>(a, LaneMax()); return a[0]; }

// row index of accumulator register `reg` of a 32x32 MFMA result in lane half `h` (guide §3)
__device__ __forceinline__ constexpr int mfma_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// A-operand fragment of M^T for v_mfma_f32_32x32x16_bf16 taken from a ROW-MAJOR bf16 tile in LDS with the gfx950 transposing
// read (ds_read_b64_tr_b16, CDNA4 guide T10): lane (r = lane&31, h = lane>>5), fragment element j holds
//   M[row0 + 8*(j>>2) + 4*h + (j&3)][col0 + r]
// i.e. exactly the k-permutation of an accumulator tile fed back as the other operand.  Per 16-lane group the instruction reads
// a 4-row x 16-column block: lane 4q+p supplies the address of row q, columns 4p..4p+3 and receives column (lane&15).
// Requirements: EXEC all ones, 8-byte aligned addresses (stride*2 and col0*2 multiples of 8).
typedef short s16x4 __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ typename Vec16<T>::type lds_tr_frag(const T* base, int stride, int row0, int col0, int lane) {
  const int i = lane & 15, g1 = (lane >> 4) & 1, h = lane >> 5;
  const T* p = base + (row0 + 4 * h + (i >> 2)) * stride + col0 + 16 * g1 + 4 * (i & 3);
  typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
  typedef typename Vec8<T>::type V4;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)p);
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 8 * stride));
  V4 l4 = __builtin_bit_cast(V4, lo), h4 = __builtin_bit_cast(V4, hi);
  typename Vec16<T>::type f;
#pragma unroll
  for (int j = 0; j < 4; ++j) { f[j] = l4[j]; f[4 + j] = h4[j]; }
  return f;
}

// erf-GELU (nn.GELU(), cod.py:854) on the VALU budget of an HBM-bound kernel.  Phi(x) = 0.5 erfc(-x/sqrt2) with erfc from
// Abramowitz-Stegun 7.1.26 evaluated on |x| so the negative tail has no 1 + erf cancellation; the exponential exp(-x^2/2) is shared
// with the Gaussian term of the derivative.  ~14 VALU ops instead of ~50 for erff + expf.  Returns Phi(x); *pdf = exp(-x^2/2) / sqrt(2 pi).
// Absolute error of Phi: <= 5e-7.  The formula itself is within 1.5e-7 of erfc (7.5e-8 on Phi); its fp32 evaluation adds about a
// dozen roundings of O(1) intermediates (v_rcp_f32, the Horner terms, which cancel near x = 0, v_exp_f32, the products, 1 - hc).
// The bound is absolute: in the far negative tail (x < -4) it is larger than Phi itself, and gelu(x) there has no relative accuracy.
__device__ __forceinline__ float gelu_phi(float x, float* pdf) {
  const float a = fabsf(x) * 0.70710678118654752f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, a, 1.f));
  const float q = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float e = __builtin_amdgcn_exp2f(-a * a * 1.4426950408889634f);
  const float hc = 0.5f * q * e;                     // 0.5 erfc(|x| / sqrt2)
  *pdf = 0.3989422804014327f * e;
  return x >= 0.f ? 1.f - hc : hc;
}
__device__ __forceinline__ float gelu_fast(float x) { float pdf; return x * gelu_phi(x, &pdf); }
__device__ __forceinline__ float gelu_grad_fast(float x) { float pdf; const float phi = gelu_phi(x, &pdf); return fmaf(x, pdf, phi); }

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// second stage of every two-stage column reduction (LayerNorm dgamma/dbeta, Linear bias gradients, layer-scale gradients): see
// dgtd_multi_reduce in elementwise.hip.  One entry = one partial buffer ws[nblocks][ncols] summed over its rows in a fixed order.
int dgtd_multi_reduce_impl(const dgtd_reduce_entry* entries, int n, hipStream_t st);
