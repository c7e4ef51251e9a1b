// wfm.hip — weighted F-measure of py_sod_metrics 1.3.1 (WeightedFmeasure, beta^2 = 1, as twig/metric/WeightedFmeasure.py calls it) on
// the device, on top of an exact nearest-foreground (Euclidean distance) transform.
//   transform (dgtd_edt_nearest), integer only, scipy.ndimage.distance_transform_edt(gt == 0, return_indices=True) with its tie rule:
//     1. column pass (one lane per column, coalesced across x): nearest foreground row of the pixel's own column, smaller row on a
//        tie, -1 for a column without foreground; written into index_out, which doubles as the scratch of the transform
//     2. row pass (one workgroup per row): the row's candidate rows staged in LDS; every lane searches outward from its own x and
//        stops once (x - j)^2 alone exceeds the best squared distance; ties go to the smallest j
//   weighting chain (dgtd_wfm):
//     a. quantise: p8 = uint8(pred * 255), gt8 > 128 (the wrappers' quantisation), min / max of p8 (integer atomics: exact)
//     b. transform of the quantised gt
//     c. weight: E = |P - gt| and Et (a background pixel takes E of its nearest foreground pixel) are formed while the tile and its
//        3-pixel halo go to LDS; 7x7 zero-padded Gaussian in fp64; MIN_E_EA, B, Ew; per-workgroup fp64 partials of count(gt),
//        sum(Ew[gt]), sum(Ew[~gt]) in a fixed order
//     d. final: one block per image adds the partials in a fixed order and forms Q
// No floating-point atomics: two launches on the same input are bit-identical.  The file is compiled with -ffp-contract=off: every
// fp64 operation rounds as NumPy's does.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int MAXW = DGTD_EDT_MAX_W;
constexpr double EPS = 2.220446049250313e-16;    // np.spacing(1)
constexpr int TW = 32, TH = 8, HALO = 3;         // weight kernel: pixels per workgroup, radius of the 7x7 window
constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;

// matlab_style_gauss2D((7, 7), sigma=5) and log(0.5) / 5, computed once in fp64 on the host and passed to the kernel by value
struct Taps {
  double k[49];
  double decay;
};

Taps make_taps() {
  Taps t;
  double mx = 0.0, sum = 0.0;
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j) {
      const double y = (double)(i - 3), x = (double)(j - 3);
      t.k[i * 7 + j] = exp(-(x * x + y * y) / (2.0 * 5.0 * 5.0));
      mx = t.k[i * 7 + j] > mx ? t.k[i * 7 + j] : mx;
    }
  for (int i = 0; i < 49; ++i) {
    if (t.k[i] < EPS * mx) t.k[i] = 0.0;
    sum = sum + t.k[i];
  }
  if (sum != 0.0)
    for (int i = 0; i < 49; ++i) t.k[i] = t.k[i] / sum;
  t.decay = log(0.5) / 5.0;
  return t;
}

// wrapper quantisation, as in sod_metrics.hip: fp32 multiply, truncation, clamped outside [0, 1]
__device__ __forceinline__ int quant8(float v) {
  const float s = v * 255.0f;
  if (!(s > 0.0f)) return 0;
  if (s >= 255.0f) return 255;
  return (int)s;
}

// mm[2 b] = 255 - min(p8), mm[2 b + 1] = max(p8) of image b (zeroed by the caller)
template <typename T>
__global__ __launch_bounds__(256) void wfm_quant_kernel(const T* __restrict__ pred, const float* __restrict__ gt, uint8_t* __restrict__ p8,
                                                        uint8_t* __restrict__ mask, uint32_t* mm, int64_t N) {
  __shared__ uint32_t s_inv_min, s_max;
  if (threadIdx.x == 0) { s_inv_min = 0; s_max = 0; }
  __syncthreads();
  const int b = blockIdx.y;
  const size_t off = (size_t)b * N;
  uint32_t inv_min = 0, mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const uint32_t v = (uint32_t)quant8(to_f(pred[off + i]));
    p8[off + i] = (uint8_t)v;
    mask[off + i] = quant8(gt[off + i]) > 128 ? 1 : 0;
    inv_min = max(inv_min, 255u - v);
    mx = max(mx, v);
  }
  atomicMax(&s_inv_min, inv_min);
  atomicMax(&s_max, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMax(&mm[2 * b], s_inv_min);
    atomicMax(&mm[2 * b + 1], s_max);
  }
}

// phase 1: cand[y][x] = row of the nearest foreground pixel of column x (the smaller row on a tie), -1 if the column has none
__global__ __launch_bounds__(64) void edt_col_kernel(const uint8_t* __restrict__ mask, int* __restrict__ cand, int H, int W) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= W) return;
  const size_t off = (size_t)blockIdx.y * H * W + x;
  const uint8_t* m = mask + off;
  int* c = cand + off;
  int up = -1;
  for (int y = 0; y < H; ++y) {
    if (m[(size_t)y * W]) up = y;
    c[(size_t)y * W] = up;
  }
  int dn = -1;
  for (int y = H - 1; y >= 0; --y) {
    if (m[(size_t)y * W]) dn = y;
    const int u = c[(size_t)y * W];
    if (dn >= 0 && (u < 0 || dn - y < y - u)) c[(size_t)y * W] = dn;
  }
}

// phase 2: row y of one image.  index holds the candidate rows on entry and the flat index of the nearest foreground pixel on
// exit (every workgroup reads and writes its own row only); -1 in both outputs for an image without foreground.
__global__ __launch_bounds__(256) void edt_row_kernel(int* __restrict__ dist2, int* __restrict__ index, int H, int W) {
  extern __shared__ int cand[];                  // [W]
  const int y = blockIdx.x;
  const size_t base = ((size_t)blockIdx.y * H + y) * W;
  for (int x = threadIdx.x; x < W; x += 256) cand[x] = index[base + x];
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += 256) {
    int best = INT_MAX, bj = -1;
    int c = cand[x];
    if (c >= 0) { best = (y - c) * (y - c); bj = x; }
    const int reach = x > W - 1 - x ? x : W - 1 - x;
    for (int d = 1; d <= reach; ++d) {
      const int dd = d * d;
      if (dd > best) break;
      int j = x - d;                             // smaller column than anything seen so far: wins a tie
      if (j >= 0 && (c = cand[j]) >= 0) {
        const int v = dd + (y - c) * (y - c);
        if (v <= best) { best = v; bj = j; }
      }
      j = x + d;                                 // larger column than anything seen so far: loses a tie
      if (j < W && (c = cand[j]) >= 0) {
        const int v = dd + (y - c) * (y - c);
        if (v < best) { best = v; bj = j; }
      }
    }
    dist2[base + x] = bj < 0 ? -1 : best;
    index[base + x] = bj < 0 ? -1 : cand[bj] * W + bj;
  }
}

// sum of K values over the 256-thread block in a fixed order (xor butterfly per wave, then waves 0..3); every thread gets the result
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red /* LDS [4 * K] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] = v[k] + __shfl_xor(v[k], o, 64);
  if (lane == 0)
    for (int k = 0; k < K; ++k) red[w * K + k] = v[k];
  __syncthreads();
  for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
  __syncthreads();
}

// one TW x TH tile of one image: partial[(b * tiles + tile) * 3] = { count(gt), sum Ew[gt], sum Ew[~gt] } of the tile
__global__ __launch_bounds__(256) void wfm_weight_kernel(const uint8_t* __restrict__ p8, const uint8_t* __restrict__ mask,
                                                         const int* __restrict__ dist2, const int* __restrict__ index,
                                                         const uint32_t* __restrict__ mm, double* __restrict__ partial, const Taps taps,
                                                         int H, int W) {
  __shared__ double lut[256];                    // _prepare_data: P = p8 / 255, min-max normalised when max != min
  __shared__ double et[LH][LW];
  __shared__ double red[4 * 3];
  const int b = blockIdx.z, t = threadIdx.x;
  const size_t off = (size_t)b * H * W;
  {
    const int mn = 255 - (int)mm[2 * b], mx = (int)mm[2 * b + 1];
    double P = (double)t / 255.0;
    if (mx != mn) P = (P - (double)mn / 255.0) / ((double)mx / 255.0 - (double)mn / 255.0);
    lut[t] = P;
  }
  __syncthreads();
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  for (int k = t; k < LH * LW; k += 256) {
    const int ly = k / LW, lx = k % LW;
    const int gy = y0 + ly - HALO, gx = x0 + lx - HALO;
    double v = 0.0;                              // zero padding (mode="constant", cval=0)
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int i = gy * W + gx;
      const int src = mask[off + i] ? i : index[off + i];     // Et: E of the nearest foreground pixel, whose gt is 1
      if (src >= 0) v = fabs(lut[p8[off + src]] - 1.0);
    }
    et[ly][lx] = v;
  }
  __syncthreads();
  const int lx = t % TW, ly = t / TW;
  const int x = x0 + lx, y = y0 + ly;
  double s[3] = {0.0, 0.0, 0.0};
  if (x < W && y < H) {
    const int i = y * W + x;
    const bool g = mask[off + i] != 0;
    double ea = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
      for (int c = 0; c < 7; ++c) ea = ea + taps.k[a * 7 + c] * et[ly + a][lx + c];
    const double e = fabs(lut[p8[off + i]] - (g ? 1.0 : 0.0));
    const double mn = (g && ea < e) ? ea : e;
    const double bw = g ? 1.0 : 2.0 - exp(taps.decay * sqrt((double)dist2[off + i]));
    const double ew = mn * bw;
    s[0] = g ? 1.0 : 0.0;
    s[1] = g ? ew : 0.0;
    s[2] = g ? 0.0 : ew;
  }
  block_sum(s, red);
  if (t == 0) {
    double* o = partial + ((size_t)b * gridDim.x * gridDim.y + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
  }
}

__global__ __launch_bounds__(256) void wfm_final_kernel(const double* __restrict__ partial, double* __restrict__ out, int tiles) {
  __shared__ double red[4 * 3];
  const int b = blockIdx.x;
  const double* p = partial + (size_t)b * tiles * 3;
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < tiles; i += 256)
    for (int k = 0; k < 3; ++k) s[k] = s[k] + p[(size_t)i * 3 + k];
  block_sum(s, red);
  if (threadIdx.x == 0) {
    double q = 0.0;                              // gt without a foreground pixel scores 0
    if (s[0] != 0.0) {
      const double tpw = s[0] - s[1], fpw = s[2];
      const double r = 1.0 - s[1] / s[0];
      const double pr = tpw / ((tpw + fpw) + EPS);
      q = 2.0 * r * pr / ((r + pr) + EPS);
    }
    out[b] = q;
  }
}

// state = { n, sum wfm } += this batch (images in order); slot = sum wfm / n
__global__ __launch_bounds__(64) void wfm_accumulate_kernel(const double* __restrict__ out, int B, double* __restrict__ state,
                                                            double* __restrict__ slot) {
  if (threadIdx.x != 0) return;
  const double n = state[0] + (double)B;
  double s = state[1];
  for (int b = 0; b < B; ++b) s = s + out[b];
  state[0] = n;
  state[1] = s;
  slot[0] = s / n;
}

constexpr size_t ALIGN = 256;
size_t up(size_t v) { return (v + ALIGN - 1) / ALIGN * ALIGN; }
int64_t tiles_of(int H, int W) { return cdiv(W, TW) * cdiv(H, TH); }

int edt_launch(const uint8_t* mask, int32_t* dist2, int32_t* index, int B, int H, int W, hipStream_t st) {
  hipLaunchKernelGGL(edt_col_kernel, dim3((unsigned)cdiv(W, 64), (unsigned)B), dim3(64), 0, st, mask, index, H, W);
  DGTD_CHECK_LAUNCH("edt_col_kernel");
  hipLaunchKernelGGL(edt_row_kernel, dim3((unsigned)H, (unsigned)B), dim3(256), (size_t)W * sizeof(int), st, dist2, index, H, W);
  DGTD_CHECK_LAUNCH("edt_row_kernel");
  return 0;
}

}  // namespace

#define WFM_SIZES_OK(name) \
  DGTD_REQUIRE(B > 0 && H > 0 && W > 0, name ": bad sizes B=%d H=%d W=%d", B, H, W); \
  DGTD_REQUIRE(W <= MAXW && H <= MAXW, name ": map of %dx%d exceeds the supported %d per side", H, W, MAXW); \
  DGTD_REQUIRE(B <= 65535, name ": batch %d exceeds 65535", B)

extern "C" int dgtd_edt_nearest(const uint8_t* gt_mask, int32_t* dist2_out, int32_t* index_out, int B, int H, int W, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (double)B * H * W * 17.0, "dgtd_edt_nearest[B=%d,%dx%d]", B, H, W);
  WFM_SIZES_OK("edt_nearest");
  DGTD_REQUIRE(gt_mask && dist2_out && index_out, "edt_nearest: null pointer");
  return edt_launch(gt_mask, dist2_out, index_out, B, H, W, (hipStream_t)s);
}

extern "C" int64_t dgtd_wfm_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t n = (size_t)B * H * W;
  return (int64_t)(up((size_t)B * 8) + 2 * up(n) + 2 * up(n * 4) + up((size_t)B * tiles_of(H, W) * 3 * 8));
}

extern "C" int dgtd_wfm(const void* pred, dgtd_dtype pred_dt, const float* gt, double* out, void* workspace, int B, int H, int W,
                        dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (double)B * H * W * (dgtd_esize(pred_dt) + 4.0 + 2.0 + 17.0 + 10.0), "dgtd_wfm[B=%d,%dx%d]", B, H, W);
  WFM_SIZES_OK("wfm");
  DGTD_REQUIRE(pred_dt == DGTD_F32 || DGTD_IS_HALF(pred_dt), "wfm: bad pred dtype %d", (int)pred_dt);
  DGTD_REQUIRE(pred && gt && out && workspace, "wfm: null pointer");
  static const Taps taps = make_taps();
  hipStream_t st = (hipStream_t)s;
  const int64_t N = (int64_t)H * W;
  const size_t n = (size_t)B * N;
  char* w = (char*)workspace;
  uint32_t* mm = (uint32_t*)w;
  w += up((size_t)B * 8);
  uint8_t* p8 = (uint8_t*)w;
  w += up(n);
  uint8_t* mask = (uint8_t*)w;
  w += up(n);
  int32_t* dist2 = (int32_t*)w;
  w += up(n * 4);
  int32_t* index = (int32_t*)w;
  w += up(n * 4);
  double* partial = (double*)w;
  if (hipMemsetAsync(mm, 0, (size_t)B * 8, st) != hipSuccess) DGTD_FAIL(3, "wfm: workspace memset failed");
  const dim3 qgrid((unsigned)(cdiv(N, 2048) < 64 ? cdiv(N, 2048) : 64), (unsigned)B);
  DGTD_DISPATCH(pred_dt, hipLaunchKernelGGL(wfm_quant_kernel<T_>, qgrid, dim3(256), 0, st, (const T_*)pred, gt, p8, mask, mm, N));
  DGTD_CHECK_LAUNCH("wfm_quant_kernel");
  if (int rc = edt_launch(mask, dist2, index, B, H, W, st)) return rc;
  const dim3 wgrid((unsigned)cdiv(W, TW), (unsigned)cdiv(H, TH), (unsigned)B);
  hipLaunchKernelGGL(wfm_weight_kernel, wgrid, dim3(256), 0, st, p8, mask, dist2, index, mm, partial, taps, H, W);
  DGTD_CHECK_LAUNCH("wfm_weight_kernel");
  hipLaunchKernelGGL(wfm_final_kernel, dim3(B), dim3(256), 0, st, partial, out, (int)tiles_of(H, W));
  DGTD_CHECK_LAUNCH("wfm_final_kernel");
  return 0;
}

extern "C" int dgtd_wfm_accumulate(const double* out, int B, double* state, double* running_slot, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (double)B * 8.0 + 2.0 * DGTD_WFM_STATE * 8.0, "dgtd_wfm_accumulate[B=%d]", B);
  DGTD_REQUIRE(B > 0, "wfm_accumulate: bad batch %d", B);
  DGTD_REQUIRE(out && state && running_slot, "wfm_accumulate: null pointer");
  hipLaunchKernelGGL(wfm_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, out, B, state, running_slot);
  DGTD_CHECK_LAUNCH("wfm_accumulate_kernel");
  return 0;
}
