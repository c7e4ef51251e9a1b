// predict_maps.hip — the output-side twin of preprocess_batch.hip: the logit maps of a batch [B,S,S] -> one grey-level prediction
// map per job, each at its own size H x W, packed as uint8 into ONE buffer (include/dgtd.h: dgtd_predict_job, offsets only).
// Replaces, per sample, F.interpolate(bilinear, align_corners=False) -> sigmoid -> mul(255) -> add(0.5) -> clamp -> to(uint8)
// (torchvision save_image's rule, the `_output.png` of twig/model/cod.py:156-217) and the min-max rule of the field's test scripts.
//
// Arithmetic, all fp32, every operation rounds (this file is compiled with contraction off), in this order per output pixel (y, x):
//   scale = (float)in / (float)out;  src = max(scale * (dst + 0.5) - 0.5, 0);  i0 = floor(src);  i1 = i0 + (i0 < in - 1);  l = src - i0
//   top = (1 - lx) * L[y0][x0] + lx * L[y0][x1];   bot = (1 - lx) * L[y1][x0] + lx * L[y1][x1];   r = (1 - ly) * top + ly * bot
//   s = 1 / (1 + expf(-r))
//   plain  : byte = floor(clamp(255 * s + 0.5, 0, 255)), NaN -> 0
//   min-max: v = (s - min s) / (max s - min s + 1e-8) over the job's own pixels (NaN pixels take no part), byte from v the same way
// Min and max are integer atomics on the ordered bit pattern of s, so they do not depend on the order of arrival; the quantise pass
// recomputes s with the very same instructions, so the pixel that set the minimum maps to exactly 0.
//
// Thread -> byte map.  blockIdx.y is the job; blockIdx.x strides over the job's UNITS.  A unit is the part of one output row that
// falls into one V-byte-aligned segment of the packed buffer (V = 16 for W >= 64, else 4): a unit that the row fills is stored as
// one dwordx4 / dword, the unaligned head and tail of a row (rows are W bytes, unpadded) as single bytes.  Row y spans at most
// U = (W + 2V - 2) / V segments; unit index = y * U + u.  The vertical taps are per unit, the horizontal taps per byte.
// HBM/latency-bound: B*S*S elements in (gathered, L2-resident), sum(H*W) bytes out.
#include "common.h"

namespace {

constexpr int MAX_SIDE = 1 << 24;
constexpr int WIDE_W = 64;     // rows at least this long take 16-byte units

__host__ __device__ __forceinline__ int unit_bytes(int W) { return W >= WIDE_W ? 16 : 4; }
__host__ __device__ __forceinline__ int units_per_row(int W, int V) { return (W + 2 * V - 2) / V; }

// F.interpolate's source index of output index dst (align_corners=False, no antialias): two taps and the weight of the second
__device__ __forceinline__ void taps(float scale, int dst, int in, int& i0, int& i1, float& lam) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;                              // src >= 0: truncation is floor
  i0 = i0 > in - 1 ? in - 1 : i0;             // never taken (src < in); keeps the reads inside the plane
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = src - (float)i0;
}

// monotone map fp32 -> uint32 (a < b  <=>  key(a) < key(b)) and back
__device__ __forceinline__ uint32_t ordered_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ uint32_t quantise(float v01) {
  float q = 255.0f * v01 + 0.5f;
  if (!(q >= 0.0f)) q = 0.0f;                 // negatives and NaN
  if (q > 255.0f) q = 255.0f;
  return (uint32_t)(int)q;
}

struct Extrema { uint32_t lo, hi; };          // ordered keys of min s and max s of one job

enum { PLAIN = 0, REDUCE = 1, MINMAX = 2 };

// one job, units of V bytes.  PLAIN / MINMAX write bytes; REDUCE folds the sigmoids into (kmin, kmax).
template <typename T, int V, int MODE>
__device__ __forceinline__ void run_job(const dgtd_predict_job& jb, const T* __restrict__ plane, uint8_t* __restrict__ out, int S, float mn, float den,
                                        uint32_t& kmin, uint32_t& kmax) {
#pragma clang fp contract(off)
  const int H = jb.H, W = jb.W;
  const int U = units_per_row(W, V);
  const int64_t units = (int64_t)H * U;
  const float sh = (float)S / (float)H, sw = (float)S / (float)W;
  for (int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x; unit < units; unit += (int64_t)gridDim.x * 256) {
    const int y = (int)(unit / U), u = (int)(unit - (int64_t)y * U);
    const int64_t row_lo = (int64_t)y * W;                                  // byte range of the row within the map: [row_lo, row_lo + W)
    const int64_t seg_lo = (row_lo & ~(int64_t)(V - 1)) + (int64_t)u * V;   // the unit's aligned segment: [seg_lo, seg_lo + V)
    const int64_t lo = seg_lo > row_lo ? seg_lo : row_lo;
    const int64_t hi = seg_lo + V < row_lo + W ? seg_lo + V : row_lo + W;
    if (lo >= hi) continue;                                                 // the segment lies past the row's end
    int y0, y1;
    float ly;
    taps(sh, y, S, y0, y1, ly);
    const T* r0 = plane + (int64_t)y0 * S;
    const T* r1 = plane + (int64_t)y1 * S;
    const float hy = 1.0f - ly;
    uint32_t bytes[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      bytes[k] = 0;
      const int64_t at = seg_lo + k;
      if (at < lo || at >= hi) continue;
      int x0, x1;
      float lx;
      taps(sw, (int)(at - row_lo), S, x0, x1, lx);
      const float hx = 1.0f - lx;
      const float top = hx * to_f(r0[x0]) + lx * to_f(r0[x1]);
      const float bot = hx * to_f(r1[x0]) + lx * to_f(r1[x1]);
      const float r = hy * top + ly * bot;
      const float s = 1.0f / (1.0f + expf(-r));
      if (MODE == REDUCE) {
        if (s == s) {                                                       // a NaN takes no part in the extrema
          const uint32_t key = ordered_key(s);
          kmin = key < kmin ? key : kmin;
          kmax = key > kmax ? key : kmax;
        }
      } else {
        bytes[k] = quantise(MODE == MINMAX ? (s - mn) / den : s);
      }
    }
    if (MODE == REDUCE) continue;
    uint8_t* dst = out + jb.out_off;
    if (lo == seg_lo && hi == seg_lo + V) {                                 // the row fills the segment: one aligned vector store
      uint32_t w[V / 4];
#pragma unroll
      for (int q = 0; q < V / 4; ++q) w[q] = bytes[4 * q] | (bytes[4 * q + 1] << 8) | (bytes[4 * q + 2] << 16) | (bytes[4 * q + 3] << 24);
      if constexpr (V == 16) *(uint4*)(dst + seg_lo) = make_uint4(w[0], w[1], w[2], w[3]);
      else *(uint32_t*)(dst + seg_lo) = w[0];
    } else {                                                                // head or tail of a row: byte stores, neighbours untouched
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (seg_lo + k >= lo && seg_lo + k < hi) dst[seg_lo + k] = (uint8_t)bytes[k];
    }
  }
}

__global__ __launch_bounds__(256) void predict_clear_kernel(Extrema* __restrict__ ext, int njobs) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < njobs) { ext[j].lo = 0xffffffffu; ext[j].hi = 0u; }
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void predict_maps_kernel(const dgtd_predict_job* __restrict__ jobs, const T* __restrict__ logits, uint8_t* __restrict__ out,
                                                           Extrema* __restrict__ ext, int S) {
#pragma clang fp contract(off)
  const dgtd_predict_job jb = jobs[blockIdx.y];
  const T* plane = logits + (int64_t)jb.batch * S * S;
  float mn = 0.f, den = 1.f;
  if (MODE == MINMAX) {
    const Extrema e = ext[blockIdx.y];
    if (e.lo <= e.hi) {                       // otherwise no pixel of the job had a number: every s is NaN and quantises to 0
      mn = ordered_value(e.lo);
      den = (ordered_value(e.hi) - mn) + 1e-8f;
    }
  }
  uint32_t kmin = 0xffffffffu, kmax = 0u;
  if (unit_bytes(jb.W) == 16) run_job<T, 16, MODE>(jb, plane, out, S, mn, den, kmin, kmax);
  else run_job<T, 4, MODE>(jb, plane, out, S, mn, den, kmin, kmax);
  if (MODE == REDUCE) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t a = (uint32_t)__shfl_xor((int)kmin, o, 64), b = (uint32_t)__shfl_xor((int)kmax, o, 64);
      kmin = a < kmin ? a : kmin;
      kmax = b > kmax ? b : kmax;
    }
    __shared__ uint32_t smin[4], smax[4];
    if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = kmin; smax[threadIdx.x >> 6] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w) { kmin = smin[w] < kmin ? smin[w] : kmin; kmax = smax[w] > kmax ? smax[w] : kmax; }
      if (kmin <= kmax) {                     // the block saw at least one number
        atomicMin(&ext[blockIdx.y].lo, kmin);
        atomicMax(&ext[blockIdx.y].hi, kmax);
      }
    }
  }
}

}  // namespace

extern "C" int64_t dgtd_predict_maps_workspace(int njobs) {
  if (njobs < 1 || njobs > DGTD_PREDICT_MAPS_MAX_JOBS) return -1;
  return ((int64_t)njobs * (int64_t)sizeof(Extrema) + 15) & ~(int64_t)15;
}

extern "C" int dgtd_predict_maps(const void* logits, dgtd_dtype dt, int B, int S, const dgtd_predict_job* jobs_dev, const dgtd_predict_job* jobs_host,
                                 int njobs, void* out_u8, int64_t out_bytes, int normalize, void* workspace, int64_t workspace_bytes, dgtd_stream s) {
  static_assert(sizeof(dgtd_predict_job) == 32, "dgtd_predict_job is 32 bytes");
  // the job is the grid's second dimension (gridDim.y <= 65535); checked before the table is read
  DGTD_REQUIRE(njobs >= 1 && njobs <= DGTD_PREDICT_MAPS_MAX_JOBS, "predict_maps: %d jobs, the grid's second dimension takes 1..%d", njobs,
               DGTD_PREDICT_MAPS_MAX_JOBS);
  int dt_code;                                 // a caller through the C ABI can pass any int: read it as one before it is used as the enum
  __builtin_memcpy(&dt_code, &dt, sizeof dt_code);
  DGTD_REQUIRE(dt_code == DGTD_F32 || dt_code == DGTD_BF16 || dt_code == DGTD_F16, "predict_maps: bad logit dtype %d", dt_code);
  DGTD_REQUIRE(normalize == 0 || normalize == 1, "predict_maps: normalize is 0 (plain) or 1 (min-max), got %d", normalize);
  DGTD_REQUIRE(logits != nullptr && jobs_dev != nullptr && jobs_host != nullptr && out_u8 != nullptr, "predict_maps: null buffer");
  DGTD_REQUIRE(B >= 1 && S >= 1 && (int64_t)S * S <= INT32_MAX, "predict_maps: bad sizes B=%d S=%d", B, S);
  DGTD_REQUIRE(out_bytes >= 1, "predict_maps: bad output size %lld", (long long)out_bytes);
  DGTD_REQUIRE(((uintptr_t)out_u8 & 15) == 0 && ((uintptr_t)jobs_dev & 7) == 0 && ((uintptr_t)logits & (uintptr_t)(dgtd_esize(dt) - 1)) == 0,
               "predict_maps: the output must be 16-byte aligned, the job table 8-byte aligned, the logits aligned to their element");
  if (normalize)
    DGTD_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 7) == 0 && workspace_bytes >= dgtd_predict_maps_workspace(njobs),
                 "predict_maps: min-max needs an 8-byte-aligned workspace of %lld bytes, got %lld", (long long)dgtd_predict_maps_workspace(njobs),
                 (long long)workspace_bytes);
  double bytes_out = 0.0;
  int64_t max_units = 0;
  for (int j = 0; j < njobs; ++j) {
    const dgtd_predict_job& jb = jobs_host[j];
    DGTD_REQUIRE(jb.H >= 1 && jb.W >= 1 && jb.H <= MAX_SIDE && jb.W <= MAX_SIDE, "predict_maps: job %d: bad size H=%d W=%d (sides 1..%d)", j, jb.H, jb.W,
                 MAX_SIDE);
    DGTD_REQUIRE(jb.reserved[0] == 0 && jb.reserved[1] == 0 && jb.reserved[2] == 0, "predict_maps: job %d: reserved fields must be 0", j);
    DGTD_REQUIRE(jb.batch >= 0 && jb.batch < B, "predict_maps: job %d: batch index %d outside [0,%d)", j, jb.batch, B);
    const int64_t map = (int64_t)jb.H * jb.W;
    DGTD_REQUIRE((jb.out_off & 15) == 0, "predict_maps: job %d: offset %lld not 16-byte aligned", j, (long long)jb.out_off);
    DGTD_REQUIRE(jb.out_off >= 0 && jb.out_off <= out_bytes - map, "predict_maps: job %d: map [%lld,+%lld) outside the %lld bytes passed in", j,
                 (long long)jb.out_off, (long long)map, (long long)out_bytes);
    bytes_out += (double)map;
    max_units = std::max<int64_t>(max_units, (int64_t)jb.H * units_per_row(jb.W, unit_bytes(jb.W)));
  }
  DGTD_PROF(s, DGTD_HBM, (double)dgtd_esize(dt) * B * S * S + bytes_out, "dgtd_predict_maps[%dx<-%d %s]", njobs, S, normalize ? "minmax" : "plain");
  hipStream_t st = (hipStream_t)s;
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(max_units, 256), 2048), (unsigned)njobs);
  uint8_t* out = (uint8_t*)out_u8;
  Extrema* ext = (Extrema*)workspace;
  if (!normalize) {
    DGTD_DISPATCH(dt, hipLaunchKernelGGL((predict_maps_kernel<T_, PLAIN>), grid, dim3(256), 0, st, jobs_dev, (const T_*)logits, out, ext, S));
    DGTD_CHECK_LAUNCH("predict_maps");
    return 0;
  }
  hipLaunchKernelGGL(predict_clear_kernel, dim3((unsigned)cdiv(njobs, 256)), dim3(256), 0, st, ext, njobs);
  DGTD_CHECK_LAUNCH("predict_maps_clear");
  DGTD_DISPATCH(dt, hipLaunchKernelGGL((predict_maps_kernel<T_, REDUCE>), grid, dim3(256), 0, st, jobs_dev, (const T_*)logits, out, ext, S));
  DGTD_CHECK_LAUNCH("predict_maps_reduce");
  DGTD_DISPATCH(dt, hipLaunchKernelGGL((predict_maps_kernel<T_, MINMAX>), grid, dim3(256), 0, st, jobs_dev, (const T_*)logits, out, ext, S));
  DGTD_CHECK_LAUNCH("predict_maps_minmax");
  return 0;
}
